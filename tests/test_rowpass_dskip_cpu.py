"""Host side of the D skip's switch (include/satrl_ppo.h
satrl_ppo_rowpass_dskip, satrl.ppo.rowpass_dskip): query, set and restore, and
the refusal's text.  No device call is made."""
import pytest


def test_dskip_switch_sets_queries_and_rejects():
    import satrl._lib as L
    from satrl.ppo import rowpass_dskip
    lib = L.lib()
    first = lib.satrl_ppo_rowpass_dskip(-1)
    assert first == 1                                   # the skip is the default
    try:
        assert lib.satrl_ppo_rowpass_dskip(0) == first  # returns the previous mode
        assert lib.satrl_ppo_rowpass_dskip(-1) == 0 and rowpass_dskip() == 0
        assert rowpass_dskip(1) == 0 and rowpass_dskip() == 1
        for bad in (2, -2, 7):
            assert lib.satrl_ppo_rowpass_dskip(bad) == -1
            msg = lib.satrl_ppo_last_error().decode()
            assert msg.startswith("satrl_ppo_rowpass_dskip:") and "mode" in msg and str(bad) in msg, msg
            assert lib.satrl_ppo_rowpass_dskip(-1) == 1  # unchanged by a refused call
        with pytest.raises(ValueError, match="rowpass_dskip"):
            rowpass_dskip(3)
        assert rowpass_dskip() == 1
    finally:
        lib.satrl_ppo_rowpass_dskip(first)


def test_dskip_switch_is_independent_of_the_sync_switch():
    from satrl.ppo import rowpass_dskip, rowpass_sync
    prev = rowpass_sync(), rowpass_dskip()
    try:
        for s in (0, 1):
            for d in (0, 1):
                rowpass_sync(s)
                rowpass_dskip(d)
                assert (rowpass_sync(), rowpass_dskip()) == (s, d)
    finally:
        rowpass_sync(prev[0])
        rowpass_dskip(prev[1])
