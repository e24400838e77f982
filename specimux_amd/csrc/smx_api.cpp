// smx_api.cpp -- host side of libsmx.so, the part every subsystem shares: the error sink, version and device selection, the
// IUPAC alphabet, the window packer and the RCCL wrappers.  The C ABI of include/smx.h is spread over this file,
// smx_panel.cpp (panel compilation, demux launch glue), smx_calls.cpp (one-shot calls) and smx_lane.cpp (lanes, statistics).
// All are compiled with hipcc.  No CPU implementation of the hot path lives in them: every compute entry point needs a HIP
// device and fails with SMX_ERR_DEVICE otherwise.
#include <rccl/rccl.h>

#include <cstdarg>

#include "smx_host.h"

namespace {

thread_local std::string g_err;

// ---- IUPAC equality (reference constants.py:13-20): symmetric, NOT transitive
struct EqTable {
    bool eq[128][128];
    EqTable() {
        memset(eq, 0, sizeof(eq));
        for (int c = 0; c < 128; c++) eq[c][c] = true;
        const char *pairs[] = {"YC", "YT", "RA", "RG", "NA", "NC", "NG", "NT", "WA", "WT", "MA", "MC", "SC", "SG",
                               "KG", "KT", "BC", "BG", "BT", "DA", "DG", "DT", "HA", "HC", "HT", "VA", "VC", "VG"};
        for (const char *p : pairs) {
            eq[(int)p[0]][(int)p[1]] = true;
            eq[(int)p[1]][(int)p[0]] = true;
        }
    }
};
const EqTable &eqt() {
    static EqTable t;
    return t;
}

}  // namespace

bool smx_iupac_eq(unsigned char a, unsigned char b) { return a < 128 && b < 128 && eqt().eq[a][b]; }

int code_of(unsigned char ch) {
    for (int c = 0; c < 15; c++)
        if (smx::kCodeChars[c] == (char)ch) return c;
    return 15;
}

unsigned char complement_of(unsigned char ch) {   // Bio.Seq complement, ambiguous DNA table, case kept, U->A
    static const char *from = "ACGTMRWSYKVHDBXNUacgtmrwsykvhdbxnu";
    static const char *to = "TGCAKYWSRMBDHVXNAtgcakywsrmbdhvxna";
    for (int i = 0; from[i]; i++)
        if ((unsigned char)from[i] == ch) return (unsigned char)to[i];
    return ch;
}

bool build_peq(const char *pat, int m, unsigned long long *peq16, std::string *bad) {
    for (int c = 0; c < 16; c++) peq16[c] = 0;
    for (int i = 0; i < m; i++) {
        unsigned char pc = (unsigned char)pat[i];
        if (pc >= 128 || code_of(pc) == 15) {
            if (bad) *bad = std::string("pattern character '") + (char)pc + "' is outside the IUPAC DNA alphabet";
            return false;
        }
        for (int c = 0; c < 15; c++)
            if (eqt().eq[pc][(int)smx::kCodeChars[c]]) peq16[c] |= 1ull << i;
    }
    return true;
}

// shared with smx_io.cpp and every host file (smx_host.h: fail): set the thread-local message and return `code`
int smx_set_error(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int smx_abi_version(void) { return SMX_ABI_VERSION; }
const char *smx_last_error(void) { return g_err.c_str(); }

int smx_device_init(int device, int *n_devices) {
    int n = 0;
    SMX_TRY(require_device(&n));
    if (n_devices) *n_devices = n;
    if (device < 0 || device >= n) return fail(SMX_ERR_ARG, "device %d out of range (0..%d)", device, n - 1);
    HIP_TRY(hipSetDevice(device));
    return SMX_OK;
}

int smx_pack_windows(const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads, int32_t S, uint8_t *windows,
                     int32_t *lens) {
    if (!bases || !offsets || !windows || !lens || S < 1) return fail(SMX_ERR_ARG, "null argument");
    const size_t stride = ((size_t)(2 * S) + 15) & ~(size_t)15;
    for (uint32_t i = 0; i < n_reads; i++) {
        uint64_t a = offsets[i], b = offsets[i + 1];
        if (b < a || b - a > 0x7FFFFFFFull) return fail(SMX_ERR_ARG, "read %u: bad offsets", i);
        int L = (int)(b - a), Sp = L < S ? L : S;
        uint8_t *w = windows + (size_t)i * stride;
        memset(w, 0, stride);
        memcpy(w, bases + a, (size_t)Sp);
        memcpy(w + S, bases + b - Sp, (size_t)Sp);
        lens[i] = L;
    }
    return SMX_OK;
}

// ---- RCCL over xGMI: one communicator per process (one process per GPU)
int smx_comm_unique_id(uint8_t id[128]) {
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    ncclUniqueId u;
    ncclResult_t r = ncclGetUniqueId(&u);
    if (r != ncclSuccess) return fail(SMX_ERR_DEVICE, "ncclGetUniqueId: %s", ncclGetErrorString(r));
    memcpy(id, &u, 128);
    return SMX_OK;
}

int smx_comm_init(const uint8_t id[128], int n_ranks, int rank, void **comm_out) {
    if (!id || !comm_out) return fail(SMX_ERR_ARG, "null argument");
    ncclUniqueId u;
    memcpy(&u, id, 128);
    ncclComm_t comm;
    ncclResult_t r = ncclCommInitRank(&comm, n_ranks, u, rank);
    if (r != ncclSuccess) return fail(SMX_ERR_DEVICE, "ncclCommInitRank: %s", ncclGetErrorString(r));
    *comm_out = (void *)comm;
    return SMX_OK;
}

int smx_counts_allreduce(uint64_t *d_counts, size_t n, void *comm, void *stream) {
    if (!d_counts || !comm) return fail(SMX_ERR_ARG, "null argument");
    ncclResult_t r = ncclAllReduce(d_counts, d_counts, n, ncclUint64, ncclSum, (ncclComm_t)comm, (hipStream_t)stream);
    if (r != ncclSuccess) return fail(SMX_ERR_DEVICE, "ncclAllReduce: %s", ncclGetErrorString(r));
    return SMX_OK;
}

void smx_comm_destroy(void *comm) {
    if (comm) (void)ncclCommDestroy((ncclComm_t)comm);
}
