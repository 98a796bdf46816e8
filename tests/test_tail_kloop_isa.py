"""The order of a k-group of tail_chain_kernel as the compiler left it (CPU only; skipped without hipcc): runs
``tools/tail_isa.py``'s ``kloops()`` on the two D = 128 fp32 rows forms test_tail_isa.py names.

* Between the last ``v_mfma`` of a k-group and the barrier that ends it (every barrier between two k-groups of stages E, B
  and C, ``tc_kgroup_barrier``) stands nothing but ``s_waitcnt lgkmcnt(..)``: no LDS store, no global load, no wait for the
  vector memory counter -- the weight stream's store, its wait and the next request run among the k-group's MFMAs.
* With stage E in front, stage B's first weights (``tc_load(.., A.wB, 0, ..)``) are requested under stage C's r_e k-groups:
  at least one k-group of stage C's MFMAs (32) lies between the request and the wait that covers it.
* With stage E in front, no load of stage A's rows is issued in front of the first store of stage C's weights (the rows
  are requested behind it: a wait for the weights in front of them is not a wait for the rows).

The form without stage E has no stage in front of stage B -- its rows and stage B's first weights are the first things the
kernel requests -- so the last two statements have nothing to say about it; what is asserted there is that the tool sees
its requests at all."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("tail_isa", os.path.join(ROOT, "tools", "tail_isa.py"))
tail_isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tail_isa)

pytestmark = pytest.mark.skipif(tail_isa.find_hipcc() is None, reason="needs hipcc")
EW, PERM = "tail_chain_kernel<8,9,16,0,true,true>", "tail_chain_kernel<8,9,16,0,true,false>"
# barriers between two k-groups of a stage: E 4 double k-groups, C over r_e 8, B 9, C over r_p 9 -- one less each, but
# for the r_e loop of the form without stage E, which the r_p loop follows directly; that form's short path has 8 more
KGROUP_BARRIERS = {EW: 3 + 7 + 8 + 8, PERM: 7 + 8 + 8 + 8}


@pytest.fixture(scope="module")
def order():
    return {k["kernel"]: k for k in tail_isa.kloops()}


@pytest.mark.parametrize("kernel", (EW, PERM))
def test_nothing_but_the_lds_wait_between_the_last_mfma_and_the_barrier(order, kernel):
    ends = order[kernel]["kgroup_ends"]
    assert len(ends) == KGROUP_BARRIERS[kernel], len(ends)
    odd = [e for e in ends if any(not (x.startswith("s_waitcnt ") and "lgkmcnt" in x and "vmcnt" not in x) for x in e)]
    assert not odd, f"{kernel}: between a k-group's last v_mfma and its barrier: {odd[:3]}"


def test_stage_b_first_weights_fly_under_a_kgroup_of_stage_c(order):
    b = order[EW]["b_first"]
    assert len(b) == 2, b                        # (two weight elements per thread and stage)
    assert all(x["mfma_to_wait"] is not None and x["mfma_to_wait"] >= 32 for x in b), b
    assert len(order[PERM]["b_first"]) == 2      # (seen; the kernel's first request, nothing to fly under)


def test_no_row_load_in_front_of_the_first_store_of_stage_c_weights(order):
    c = order[EW]["c_first_store"]
    assert c is not None and c["rows_in_front"] == 0, c
    assert order[PERM]["c_first_store"] is not None
