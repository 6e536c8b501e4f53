#!/bin/bash
cd "$GRAFT_REPO_ROOT" || exit 1
O=gpurun_out/r6_wave3; mkdir -p $O
timeout 900 python -m pytest tests/test_gpu_wave.py -x -q -s > $O/pytest_wave.txt 2>&1; echo "pytest wave rc $?" | tee $O/summary.txt
tail -8 $O/pytest_wave.txt
B2T_WAVE_LOCAL=0 timeout 900 python -m pytest tests/test_gpu_wave.py -x -q > $O/pytest_wave_nolocal.txt 2>&1; echo "pytest wave (placement-independent form) rc $?" | tee -a $O/summary.txt
timeout 600 python tools/r6_wave_probe.py > $O/probe_local.txt 2>&1; grep "R6WAVE\|R6STALE" $O/probe_local.txt | tee -a $O/summary.txt; tail -3 $O/probe_local.txt
B2T_LIB=$PWD/nejm-brain-to-text_amd/csrc/libb2t_hip_wtiming.so timeout 600 python tools/r6_wave_probe.py > $O/probe_timing.txt 2>&1; grep "R6WAVE" $O/probe_timing.txt | tee -a $O/summary.txt
B2T_WAVE_LOCAL=0 B2T_LIB=$PWD/nejm-brain-to-text_amd/csrc/libb2t_hip_wtiming.so timeout 600 python tools/r6_wave_probe.py > $O/probe_timing_nolocal.txt 2>&1; grep "R6WAVE" $O/probe_timing_nolocal.txt | tee -a $O/summary.txt
python tools/r6_amp_ab.py 2>/dev/null | grep R6AMP | tee -a $O/summary.txt
