"""Host side of the rowpass synchronisation switch (include/satrl_ppo.h
satrl_ppo_rowpass_sync) and of the 32-row kernel's direct entry
(satrl_ppo_rowpass_kx32): no device call is made."""
import ctypes as C


def test_rowpass_sync_switch_sets_queries_and_rejects():
    import satrl._lib as L
    from satrl.ppo import rowpass_sync
    lib = L.lib()
    first = lib.satrl_ppo_rowpass_sync(-1)
    assert first == 1                                   # the hand-off form is the default
    try:
        assert lib.satrl_ppo_rowpass_sync(0) == first   # returns the previous mode
        assert lib.satrl_ppo_rowpass_sync(-1) == 0 and rowpass_sync() == 0
        assert rowpass_sync(1) == 0 and rowpass_sync() == 1
        for bad in (2, -2, 7):
            assert lib.satrl_ppo_rowpass_sync(bad) == -1
            assert lib.satrl_ppo_rowpass_sync(-1) == 1  # unchanged by a refused call
    finally:
        lib.satrl_ppo_rowpass_sync(first)


def test_uses_handoff_follows_the_switch():
    from satrl.ppo import rowpass_sync, uses_handoff
    prev = rowpass_sync()
    try:
        rowpass_sync(1)
        assert uses_handoff(256, 4096, 8192) and uses_handoff(256, 4096, 1025)   # one minibatch of the whole 1025 rows
        assert not uses_handoff(256, 512, 8192) and not uses_handoff(256, 4096, 700) and not uses_handoff(64, 4096, 8192)
        rowpass_sync(0)
        assert not uses_handoff(256, 4096, 8192)
    finally:
        rowpass_sync(prev)


def test_rowpass_kx32_rejects_bad_arguments_before_any_device_call():
    import satrl._lib as L
    lib = L.lib()
    fake = C.c_void_p(16)                                # never touched: every call fails its host checks
    kx = lib.satrl_ppo_kx_elems(256, 40)
    assert kx == 2 * 3 * 64 * 256
    args = [fake, None, fake, fake, 0.1, 0.01, 1.6, fake, fake, kx, fake, fake, None, None]
    assert lib.satrl_ppo_rowpass_kx32(64, 40, -1, *args) == -1                  # H 256 only
    assert lib.satrl_ppo_rowpass_kx32(256, 0, -1, *args) == -1                  # empty minibatch
    assert lib.satrl_ppo_rowpass_kx32(256, 40, 2, *args) == -1                  # net not -1/0/1
    assert lib.satrl_ppo_rowpass_kx32(256, 40, -1, None, *args[1:]) == -1       # null rows
    assert lib.satrl_ppo_rowpass_kx32(256, 40, -1, *args[:9], kx - 1, *args[10:]) == -1   # undersized planes
    assert b"planes hold" in lib.satrl_ppo_last_error()
