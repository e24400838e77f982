// AddressSanitizer / UBSan driver for the alignment kernels' lane bodies (specimux_amd/csrc/smx_align_lane.h, compiled for
// the host by tests/cpu/align_host.h): the wrap families and the exhaustive set of tests/cpu/align_sim.cpp, over heap
// buffers of exactly the sizes smx_align and smx_align_batch allocate -- tlen score bytes and tlen starts for one alignment,
// toff[n] score bytes and n * cap locations (none where cap == 0) for a launch -- so that any index the calls did not
// budget for is a heap overflow.  Every result is still held against the full-matrix reference.  CPU only; built and run
// by tests/test_align_asan.py with g++ -fsanitize=address,undefined.
#include "../cpu/align_host.h"

using namespace align_host;

int main() {
    Stats S, W;
    check_alphabet(S);
    std::thread wrap(run_wrap, std::ref(W));   // beside the exhaustive set's threads
    run_exhaustive(S);
    wrap.join();
    S.count["wrap_k_ge_m"] = W.count["k_ge_m_hw"] + W.count["k_ge_m_shw"];
    S.mismatches += W.mismatches;
    for (const auto &kv : W.count) S.count[kv.first] += kv.second;
    for (auto &kv : S.count) printf("%s %lld\n", kv.first.c_str(), kv.second);
    printf("%lld mismatches\n", S.mismatches);
    return 0;
}
