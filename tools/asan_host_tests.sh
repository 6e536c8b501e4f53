#!/bin/bash
# The CPU test suite against the library's HOST half built with AddressSanitizer (every source compiled --offload-host-only;
# the fat binaries the host stubs refer to are stood in for by zero words -- no kernel is launched by `-m "not gpu"` tests).
# Round 5, last session: 190 passed, no report.
set -e
cd "$(dirname "$0")/.."
CL=/opt/rocm/lib/llvm/bin/clang++
RT=$(find /opt/rocm/lib/llvm/lib/clang -name "libclang_rt.asan-x86_64.so" | head -1)
C=nejm-brain-to-text_amd/csrc
O=/tmp/b2t_asan_obj; rm -rf $O; mkdir -p $O
for f in gemm.hip gemm_bf16.hip gemm_bf16p.hip elementwise.hip gru.hip gru_persistent.hip ctc.hip optimizer.hip decode.hip beam.hip wfst.hip wfst_cluster.hip wfst_prune.hip wfst_lattice.hip stream.hip core.cpp exec.cpp lattice.cpp graphc.cpp; do
  $CL -x hip --offload-host-only --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -fsanitize=address -shared-libsan -Iinclude -I$C -c $C/$f -o $O/${f%.*}.o &
done
wait
$CL -fsanitize=address -shared-libsan -shared -fPIC -o /tmp/libb2t_asan_full.so $O/*.o -L/opt/rocm/lib -lamdhip64 2>/dev/null || true
( echo '// stand-ins for the fat binaries of a host-only build (never launched)'
  nm -u /tmp/libb2t_asan_full.so 2>/dev/null | grep __hip_fatbin | awk '{print $2}' | sort -u | while read s; do echo "extern \"C\" const unsigned long long $s[8] = {0,0,0,0,0,0,0,0};"; done ) > $O/fatstub.cpp
g++ -c -fPIC $O/fatstub.cpp -o $O/fatstub.o
$CL -fsanitize=address -shared-libsan -shared -fPIC -o /tmp/libb2t_asan_full.so $O/*.o -L/opt/rocm/lib -lamdhip64
B2T_LIB=/tmp/libb2t_asan_full.so LD_PRELOAD=$RT ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0" python -m pytest tests -q -m "not gpu" -p no:cacheprovider "$@"
