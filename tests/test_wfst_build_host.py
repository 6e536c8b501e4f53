"""Host: what the compiler makes of the WFST decoder's units (csrc/wfst.hip, wfst_cluster.hip, wfst_prune.hip, wfst_lattice.hip).
No GPU: the kernels are compiled for gfx950 and only their resource remarks are read."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
WFST_UNITS = ["wfst.hip", "wfst_cluster.hip", "wfst_prune.hip", "wfst_lattice.hip"]


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_wfst_kernels_do_not_spill_and_fit_a_1024_thread_workgroup():
    # The searchers and the pruning kernels run as 1024-thread workgroups (16 waves, 4 per SIMD): above 128 VGPRs they cannot be
    # launched at all, and scratch is the symptom of a struct (Lay / Graph / Opts) that reached a helper by reference -- every
    # access then becomes a FLAT instruction (csrc/wfst_prune.hip, prune_frame).  At the time of writing: scratch 0 everywhere,
    # at most 123 VGPRs (wfst_prune_kernel), the cluster searcher 104.
    import wave_kernel_resources as W
    res = {}
    for unit in WFST_UNITS:
        r = {k: v for k, v in W.resources(src=unit).items() if "wfst_" in k}
        assert r, unit
        assert not set(r) & set(res), (unit, sorted(set(r) & set(res)))      # a kernel lives in ONE unit
        res.update(r)
    cluster = [k for k in res if "wfst_cluster_kernel" in k]
    assert len(res) == 15 and len(cluster) == 4, sorted(res)
    expected = {"wfst_reset_kernel", "wfst_search_kernel", "wfst_best_path_kernel", "wfst_xcd_probe_kernel", "wfst_finalize_kernel",
                "wfst_finalize_cluster_kernel", "wfst_prune_kernel", "wfst_prune_cluster_kernel", "wfst_lattice_count_kernel",
                "wfst_lattice_ids_kernel", "wfst_lattice_arcs_kernel"}
    assert set(res) - set(cluster) == expected, sorted(res)
    spilled = {k: v for k, v in res.items() if v.get("ScratchSize", -1) != 0}
    assert not spilled, spilled
    assert all(0 <= v.get("VGPRs", -1) <= 128 for v in res.values()), res
