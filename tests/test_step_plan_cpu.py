"""The library's plan of a minibatch step (include/satrl_ppo.h
satrl_ppo_step_plan) against the size queries of the ABI, its own capacity
claims and the kernel each (H, mb, net) runs.  Host arithmetic only: no device
call is made."""
import ctypes as C

import pytest

WIDTHS = (64, 128, 256)
NETS = (-1, 0, 1)
MBS = range(1, 4201)


@pytest.fixture(scope="module")
def plans():
    """{(H, net): [plan of mb 1, plan of mb 2, ...]}, computed once (of the
    fields only the H 256 rowpass above the 16-row range follows the
    synchronisation switch; the tests below read it from fresh plans)."""
    from satrl.ppo import step_plan
    return {(H, net): [step_plan(H, mb, net) for mb in MBS] for H in WIDTHS for net in NETS}


def test_plan_equals_the_size_queries(plans):
    import satrl._lib as L
    lib = L.lib()
    nwg, nblk = C.c_int64(), C.c_int64()
    for (H, net), ps in plans.items():
        for mb, p in zip(MBS, ps):
            at = (H, mb, net)
            assert lib.satrl_ppo_sizes(H, mb, C.byref(nwg), C.byref(nblk)) == 0
            assert (p.slab_blocks, p.norm_blocks) == (nwg.value, nblk.value), at
            assert p.row_blocks == lib.satrl_ppo_row_blocks(H, mb), at
            assert p.row_blocks == -(-mb // p.rows_per_block), at
            want = (lib.satrl_ppo_row_blocks(H, mb) if p.step == L.STEP_FUSED else
                    lib.satrl_ppo_dw2_splits(H, mb) if p.step == L.STEP_ROWS else
                    lib.satrl_ppo_dw2_kx_splits(H, mb, net))
            assert p.splits == want and want >= 1, at
            assert p.kx_elems == max(lib.satrl_ppo_kx_elems(H, mb), 0), at
            assert (lib.satrl_ppo_kx_elems(H, mb) == -1) == (p.step != L.STEP_KX), at


def test_capacities_hold_every_shorter_minibatch(plans):
    for (H, net), ps in plans.items():
        top_s = top_b = 0
        for mb, p in zip(MBS, ps):
            top_s, top_b = max(top_s, p.splits), max(top_b, p.row_blocks)
            assert p.max_splits >= top_s, (H, mb, net, p.max_splits, top_s)
            assert p.slab_blocks >= top_b, (H, mb, net, p.slab_blocks, top_b)
    # the buffers as they were before the plan stated them
    pinned = {(256, 4096): 8, (256, 512): 8, (256, 33): 8, (128, 17): 32, (128, 4096): 32, (64, 17): 1,
              (64, 4096): 128}
    for (H, mb), want in pinned.items():
        assert plans[H, -1][mb - 1].max_splits == want, (H, mb)
    assert plans[256, -1][1025 - 1].slab_blocks == 64


def test_buffer_sizes(plans):
    for (H, net), ps in plans.items():
        for mb, p in zip(MBS, ps):
            assert p.ptail_floats == p.slab_blocks * (6 * H + 12), (H, mb, net)
            assert p.pw1_floats == p.slab_blocks * 2 * H * 20, (H, mb, net)
            assert p.p2_floats == 2 * p.max_splits * H * H, (H, mb, net)
            assert p.rows_floats == 2 * mb * H, (H, mb, net)


def test_step_and_rowpass_kinds(plans):
    import satrl._lib as L
    from satrl.ppo import rowpass_sync, step_plan

    def kind(H, mb, net=-1):
        p = step_plan(H, mb, net)
        return p.rowpass, p.error_word

    for (H, net), ps in plans.items():
        assert {p.step for p in ps} == {{64: L.STEP_FUSED, 128: L.STEP_ROWS, 256: L.STEP_KX}[H]}
        if H != 256:
            assert {(p.rowpass, p.error_word, p.rows_per_block) for p in ps} == {(L.RP_WG32, 0, 32)}
    prev = rowpass_sync()
    try:
        for sync, long_rows in ((1, (L.RP_WG32_HANDOFF, 1)), (0, (L.RP_WG32, 0))):
            rowpass_sync(sync)
            for mb in (1, 512, 1024):
                assert kind(256, mb) == (L.RP_CS, 1)
                assert step_plan(256, mb).rows_per_block == 16
            assert kind(256, 512, 0) == (L.RP_WG16, 0) and kind(256, 512, 1) == (L.RP_WG16, 0)
            for mb in (1025, 4096):
                for net in NETS:
                    assert kind(256, mb, net) == long_rows
                assert step_plan(256, mb).rows_per_block == 32
            for H in (64, 128):
                assert kind(H, 512) == (L.RP_WG32, 0) and kind(H, 4096) == (L.RP_WG32, 0)
    finally:
        rowpass_sync(prev)


def test_update_predicates_follow_the_plan():
    """uses_column_split / uses_handoff (an update's full minibatch and ragged
    tail) are the plan's rowpass kinds, and an unsupported width or an empty
    update has neither."""
    from satrl.ppo import uses_column_split, uses_handoff
    for H in WIDTHS + (100,):
        for mb, B in ((512, 8192), (1024, 1024), (1025, 8192), (4096, 8192), (4096, 8292), (4096, 700), (4096, 1025),
                      (4096, 10192), (0, 8192), (512, 0)):
            full = min(mb, B)
            tail = B % full if full > 0 else 0
            assert uses_column_split(H, mb, B) == (H == 256 and full > 0 and (full <= 1024 or 0 < tail <= 1024))
            assert uses_handoff(H, mb, B) == (H == 256 and full > 1024)


def test_bad_arguments():
    import satrl._lib as L
    from satrl.ppo import step_plan
    lib, p = L.lib(), L.StepPlan()
    assert lib.satrl_ppo_step_plan(100, 64, -1, C.byref(p)) == -1
    assert lib.satrl_ppo_step_plan(256, 0, -1, C.byref(p)) == -1
    assert lib.satrl_ppo_step_plan(256, 64, 2, C.byref(p)) == -1
    assert lib.satrl_ppo_step_plan(256, 64, -1, None) == -1
    assert lib.satrl_ppo_step_plan(256, 64, -1, C.byref(p)) == 0
    with pytest.raises(ValueError):
        step_plan(100, 64)
