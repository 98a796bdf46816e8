"""The weight prefetch of tail_chain_kernel as the compiler scheduled it (CPU only; skipped without hipcc): runs
tools/tail_isa.py.  In the two D = 128 fp32 rows forms -- with stage E (the three-launch step) and without -- every
steady-state weight-stage load of stages E, B and C must have at least one k-group's MFMAs (4 TPW of its stage) between its
issue and the ``s_waitcnt`` that covers it; a stage's first load is exempt.  Both kernels: no scratch, at most 128 VGPRs,
at most 81,920 B of LDS (two workgroups share a CU)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("tail_isa", os.path.join(ROOT, "tools", "tail_isa.py"))
tail_isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tail_isa)

pytestmark = pytest.mark.skipif(tail_isa.find_hipcc() is None, reason="needs hipcc")
KERNELS = ("tail_chain_kernel<8,9,16,0,true,true>", "tail_chain_kernel<8,9,16,0,true,false>")
TPW = {"E": 4, "B": 5, "C": 8}       # (NTPA, NTPB, NTPC) / 2 at D = 128


@pytest.fixture(scope="module")
def report():
    res = {k["kernel"]: k for k in tail_isa.run()}
    print(tail_isa.report(list(res.values())))
    return res


@pytest.mark.parametrize("kernel", KERNELS)
def test_weight_loads_fly_under_a_kgroup_of_mfmas(report, kernel):
    k = report[kernel]
    steady = [l for l in k["loads"] if l["steady"] and l["stage"] in TPW]
    stages = {l["stage"] for l in steady}
    assert stages == ({"E", "B", "C"} if kernel == KERNELS[0] else {"B", "C"}), stages
    # (every call site is there: E 3 stages, B 8 k-groups, C 8 r_p k-groups + the rolled r_e loop, two loads per thread)
    assert len(steady) >= 2 * (8 + 8 + 1) + (2 * 3 if "E" in stages else 0), len(steady)
    short = [(l["line"], l["stage"], l["mfma_to_wait"]) for l in steady
             if l["mfma_to_wait"] is None or l["mfma_to_wait"] < 4 * TPW[l["stage"]]]
    assert all(l["need"] == 4 * TPW[l["stage"]] for l in steady)
    assert not short, f"{kernel}: weight loads awaited before a k-group of MFMAs (line, stage, v_mfma): {short}"


@pytest.mark.parametrize("kernel", KERNELS)
def test_resources(report, kernel):
    k = report[kernel]
    assert k["scratch"] == 0 and k["vgprs"] <= 128 and k["lds"] <= 81920, (k["scratch"], k["vgprs"], k["lds"])
