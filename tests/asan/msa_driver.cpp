// AddressSanitizer / UBSan driver for the host side of smx_msa: the plan of a call (smx_msa_plan.h: the argument checks, the
// levels, the buffer sizes, the cutting of a level) and the kernels' bodies as host loops (tests/cpu/msa_host.h over
// smx_msa_core.h), run the way smx_msa.hip indexes its buffers, over heap blocks of exactly the planned sizes, so that any
// index the plan did not budget for -- a profile column, a map entry, a direction word, an op, a hand-over score, a length
// or a cost -- is a heap overflow.  Pairs at the edges of a direction word, a band and the walk's tile, very unequal
// pairs, and trees of 2 .. 9 tips, ladder and balanced, whole and cut into launches of one merge; the three visiting
// orders.  CPU only; built and run by tests/test_msa_asan.py with g++ -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../cpu/msa_host.h"

using namespace smx;

static void die(const char *what) { fprintf(stderr, "driver: %s\n", what); exit(2); }

static unsigned long long calls = 0, refusals = 0, overflows = 0;
static MsaCounters K;

static void run(std::mt19937 &rng, const std::vector<std::string> &seqs, const std::vector<smx_msa_merge> &merges, uint64_t budget) {
    const uint32_t n = (uint32_t)seqs.size();
    size_t total = 0;
    for (const std::string &s : seqs) total += s.size();
    char *blob = new char[total ? total : 1];            // exactly the sequences: nothing behind them may be read
    uint64_t *off = new uint64_t[n + 1];
    off[0] = 0;
    for (uint32_t i = 0; i < n; i++) {
        memcpy(blob + off[i], seqs[i].data(), seqs[i].size());
        off[i + 1] = off[i] + seqs[i].size();
    }
    smx_msa_merge *m = new smx_msa_merge[merges.size() ? merges.size() : 1];
    for (size_t t = 0; t < merges.size(); t++) m[t] = merges[t];
    const uint32_t X = 1 + rng() % 5, G = 1 + rng() % 5;
    MsaHostResult first;
    for (MsaOrder order : {MSA_FORWARD, MSA_REVERSED, MSA_SHUFFLED}) {
        MsaHostResult got;
        std::string why;
        if (msa_host_call(blob, off, n, m, X, G, SMX_MSA_MAX_COLS, budget, order, 7u + n, &got, &K, &why) != SMX_OK)
            die(why.c_str());
        if (got.lens.size() != merges.size() || got.rows.size() != (size_t)n * got.n_cols) die("sizes");
        for (uint32_t i = 0; i < n; i++) {                 // a row with the gaps removed is the input
            std::string back;
            for (uint32_t c = 0; c < got.n_cols; c++)
                if (got.rows[(size_t)i * got.n_cols + c] != '-') back.push_back((char)got.rows[(size_t)i * got.n_cols + c]);
            if (back != seqs[i]) die("a row is not its sequence");
        }
        calls++;
        if (order == MSA_FORWARD) first = got;
        else if (got.n_cols != first.n_cols || got.rows != first.rows || got.lens != first.lens || got.costs != first.costs)
            die("the visiting order changed the result");
    }
    if (n >= 2) {                                          // one column too few: the lengths and costs, no rows
        MsaHostResult got;
        std::string why;
        if (msa_host_call(blob, off, n, m, X, G, first.n_cols - 1, budget, MSA_FORWARD, 3u, &got, nullptr, &why) != SMX_ERR_OVERFLOW ||
            got.n_cols != first.n_cols || !got.rows.empty())
            die("overflow");
        overflows++;
        MsaPlan P;
        uint8_t rows = 0;
        uint32_t n_cols = 0, lens = 0;
        uint64_t costs = 0;
        const smx_msa_merge keep = m[merges.size() - 1];
        m[merges.size() - 1].a = m[merges.size() - 1].b;   // a == b
        if (msa_plan(blob, off, n, m, 1, 1, &rows, &n_cols, &lens, &costs, &P, &why) != SMX_ERR_ARG) die("a bad merge accepted");
        m[merges.size() - 1] = keep;
        refusals++;
    }
    delete[] blob; delete[] off; delete[] m;
}

static std::string random_seq(std::mt19937 &rng, size_t len) {
    std::string s(len, 'A');
    for (char &c : s) c = "ACGTN"[rng() % 5];
    return s;
}

int main() {
    std::mt19937 rng(5);
    run(rng, {}, {}, MSA_DEFAULT_BUDGET);
    run(rng, {random_seq(rng, 9)}, {}, MSA_DEFAULT_BUDGET);
    const uint32_t pairs[][2] = {{1, 1}, {1, 300}, {300, 3}, {15, 17}, {16, 16}, {17, 33}, {63, 65}, {64, 64}, {65, 129}, {257, 258}};
    for (const auto &p : pairs) {
        std::string a = random_seq(rng, p[0]), b = p[0] == p[1] ? a : random_seq(rng, p[1]);
        if (p[0] == p[1]) b[p[1] / 2] = b[p[1] / 2] == 'A' ? 'C' : 'A';
        run(rng, {a, b}, {{0, 1}}, MSA_DEFAULT_BUDGET);
    }
    for (uint32_t n = 2; n <= 9; n++)
        for (int kind = 0; kind < 2; kind++) {
            std::vector<std::string> seqs;
            const std::string root = random_seq(rng, 40 + 7 * n);
            for (uint32_t i = 0; i < n; i++) {
                std::string s = root;
                s.erase(rng() % s.size(), 1 + rng() % 5);
                s[rng() % s.size()] = 'T';
                seqs.push_back(s);
            }
            std::vector<smx_msa_merge> merges;
            if (kind == 0) {
                uint32_t top = 0;
                for (uint32_t i = 1; i < n; i++) { merges.push_back({top, i}); top = n + (uint32_t)merges.size() - 1; }
            } else {
                std::vector<uint32_t> live(n);
                std::iota(live.begin(), live.end(), 0u);
                while (live.size() > 1) {
                    std::vector<uint32_t> next;
                    for (size_t k = 0; k < live.size(); k += 2)
                        if (k + 1 < live.size()) { merges.push_back({live[k], live[k + 1]}); next.push_back(n + (uint32_t)merges.size() - 1); }
                        else next.push_back(live[k]);
                    live = next;
                }
            }
            run(rng, seqs, merges, MSA_DEFAULT_BUDGET);
            run(rng, seqs, merges, 1);
        }
    printf("calls %llu merges %llu launches %llu cells %llu tiles %llu overflows %llu refusals %llu\n", calls,
           (unsigned long long)K.merges, (unsigned long long)K.launches, (unsigned long long)K.cells, (unsigned long long)K.tiles,
           overflows, refusals);
    return 0;
}
