"""The pop of the hand-written packet walk tests its stack pointer ONCE since round 12 (L_pop, glome_amd/csrc/bih_packet_asm.hpp): m0 - 1 in 32
unsigned bits is >= CAP both for an entry beyond the LDS part and for an empty stack (0xffffffff), and only the slow label tells the two
apart.  tests/dispatch_model.py holds that arithmetic (pop_fold) and a 64-lane model of the block around it; here, without a GPU,

  * pop_fold is the parent's two tests (empty first, then beyond the LDS part) on every stack pointer a walk can hold and on the extremes;
  * the block entered with phase = 1 and sp = 0 -- which bih_tri_packet_hw never does (tests/test_dispatch_sites_host.py says why) -- leaves
    with status 0, am = 0 and sp = 0, in both modes;
  * on every packet of tests/test_dispatch_sites_host.py the model built on it has packet_model.walk_packet's stack pointer (its deepest, and 0 at
    every end), status (as many exits with 1 and with 3 as walk_packet pushes and pops beyond the LDS part, one exit with 0 per walk) and final
    am (no lane), and its per-lane results."""
import numpy as np

import dispatch_model as DM
import packet_model as PM
from test_dispatch_sites_host import scenes_  # noqa: F401  (the fixture: the GPU test's scenes and streams)

CAP = DM.CAP


def parents_pop(m0, cap=CAP):
    """the pop's head before round 12: s_sub_u32 m0, m0, 1; s_cbranch_scc1 L_empty (SCC = the borrow); s_cmp_ge_u32 m0, cap; s_cbranch_scc1 L_popslow"""
    borrow = m0 == 0
    m0 = (m0 - 1) & DM.U32
    if borrow:
        return "empty", 0
    if m0 >= cap:
        return "over", m0 + 1
    return "lds", m0


def test_one_compare_is_the_parents_two():
    for cap in (1, CAP, 255):
        for m0 in list(range(0, cap + 40)) + [2 ** 31 - 1, 2 ** 31, DM.U32 - 1]:
            assert DM.pop_fold(m0, cap) == parents_pop(m0, cap), (cap, m0)
    assert DM.pop_fold(0) == ("empty", 0) and DM.pop_fold(1) == ("lds", 0) and DM.pop_fold(CAP) == ("lds", CAP - 1) and DM.pop_fold(CAP + 1) == ("over", CAP + 1)
    # (m0 - 1 is 0xffffffff for m0 = 0 alone: the two forms differ on no value at all)
    assert DM.pop_fold(DM.U32) == ("over", DM.U32) == parents_pop(DM.U32)


def test_phase_1_on_an_empty_stack_is_the_end(scenes_):
    s = scenes_[-1]
    o, d = (a[:64].astype(np.float64) for a in s.streams["outside"])
    for mode in (1, 2):
        ev = []
        w = DM._Walk(s.bih, o, d, 1.0 / d, 7, np.ones(64, bool), np.zeros(64), np.full(64, 1e6), mode, np.full(64, PM.NO_BEST), np.full(64, -1, np.int64), np.zeros(64, bool), ev)
        assert w.block(1, False) == 0 and w.sp == 0 and not w.am.any()
        assert ev == [DM.Entry(1, 0, mode), DM.Pop(0, "empty", mode)]


def test_the_model_has_packet_models_stack_pointer_status_and_final_am(scenes_):
    packets = over = 0
    for s in scenes_:
        for name, mode, res in s.events():  # (asserts pushes and pops beyond the LDS part, the deepest stack pointer and the per-lane results against walk_packet)
            for r in res:
                exits = [e for e in r["events"] if isinstance(e, DM.Exit)]
                walks = sum(isinstance(e, DM.Entry) and e.phase == 0 and e.sp == 0 for e in r["events"])
                done = [e for e in exits if e.status == 0]
                assert len(done) == walks and all(e.sp == 0 and e.lanes == 0 for e in done)
                assert all(e.sp >= CAP and e.lanes > 0 for e in exits if e.status == 1) and all(e.sp > CAP for e in exits if e.status == 3)
                assert {e.status for e in exits} <= {0, 1, 3} and exits[-1].status == 0
                packets += 1; over += r["exits_pop"]
    print("packets:", packets, "exits with status 3:", over)
    assert packets > 200 and over > 100
