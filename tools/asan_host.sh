#!/bin/bash
# Host-side AddressSanitizer run of libsmx (panel compiler, window packer, streaming I/O) through the Python binding.
# CPU only (device code is compiled normally; GPU ASan is not available on this pool).  A few minutes, most of it the build.
#   tools/asan_host.sh            -> builds build_exp/libsmx_asan.so and runs the CPU host tests against it
# The library is built by csrc/Makefile with its own object directory, as `make exp` does: every source of libsmx.so is in it.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$ROOT/build_exp"
make -C "$ROOT/specimux_amd/csrc" -j"${JOBS:-8}" OBJD="$ROOT/build/smx_asan" OUT="$ROOT/build_exp/libsmx_asan.so" \
    EXTRA="-O1 -g -fsanitize=address -fno-omit-frame-pointer -Wno-option-ignored"
RT=$(/opt/rocm/lib/llvm/bin/clang -print-file-name=libclang_rt.asan-x86_64.so)
cd "$ROOT"
LD_PRELOAD=$RT ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 SMX_LIB="$ROOT/build_exp/libsmx_asan.so" \
    python -m pytest tests/test_host_cpu.py tests/test_native_io_cpu.py -x -q
