"""CPU checks of the C-ABI boundary: the library loads and exports every
symbol the public headers declare (no compute calls: no GPU here)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    return set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\**(sat\w+)\s*\(", txt, re.M))


def test_headers_declare_expected_entry_points():
    env = _declared("satenv.h")
    assert {"satenv_create", "satenv_reset", "satenv_step", "satenv_step_autoreset", "satenv_destroy",
            "satenv_get_state", "satenv_set_state", "satenv_last_error"} <= env
    assert {"satrl_gae", "satrl_gaussian_sample", "satrl_moments"} <= _declared("satrl_rollout.h")
    assert {"satrl_ppo_rowpass", "satrl_ppo_reduce", "satrl_ppo_adam", "satrl_ppo_layout"} <= _declared("satrl_ppo.h")
    assert {"satrl_peer_alloc", "satrl_peer_open", "satrl_ppo_allreduce_peer"} <= _declared("satrl_peer.h")
    # the host build exports every env entry point of satenv.h it restates, same signature, satenv_cpu_ prefix
    cpu = _declared("satenv_cpu.h")
    assert {n.replace("satenv_", "satenv_cpu_", 1) for n in ("satenv_create", "satenv_destroy", "satenv_num_envs",
            "satenv_set_params", "satenv_reset", "satenv_step", "satenv_step_autoreset", "satenv_get_state",
            "satenv_set_state", "satenv_danger_zone", "satenv_check", "satenv_last_error")} == cpu


def test_library_exports_every_declared_symbol():
    import satrl._lib as L
    if not os.path.exists(L.LIB_PATH):
        L.build()
    lib = L.lib()          # loads with torch's HIP runtime; no device needed
    declared = (_declared("satenv.h") | _declared("satenv_cpu.h") | _declared("satrl_rollout.h") |
                _declared("satrl_ppo.h") | _declared("satrl_peer.h"))
    for name in sorted(declared):
        assert hasattr(lib, name), name
    assert set(L.exported_symbols()) == declared


def test_host_helpers_without_gpu():
    import numpy as np
    import satrl._lib as L
    from satrl import env as E
    assert L.lib().satenv_abi_version() == 2
    p = E.default_params()
    assert p.max_episode_steps == 1000 and p.fuel_c0 == 320 and p.d_range == 100000
    # host STM equals the oracle's / reference's matrix bit for bit
    import oracle as O
    assert np.array_equal(E.stm(100.0), O.stm(100.0))


def _slot(lib):
    """The satrl_* error slot; both accessors return it."""
    msg = lib.satrl_last_error()
    assert lib.satrl_ppo_last_error() == msg
    return msg


def _poison(lib, name):
    """Leave another entry point's refusal in the slot, so that a refusal of
    `name` that writes nothing cannot pass for one that names itself."""
    other = "satrl_moments" if name == "satrl_gae" else "satrl_gae"
    args = (0, None, None, None) if other == "satrl_moments" else (0, 0, None, None, None, 0.0, 0.0, None, None, None)
    assert getattr(lib, other)(*args) == -1
    assert _slot(lib).startswith(other.encode() + b": ")


def _refused(lib, name, *args, code=-1, words=()):
    """`name(*args)` returns `code` and leaves "<name>: <reason>" with every one of `words` in the reason."""
    _poison(lib, name)
    assert getattr(lib, name)(*args) == code, (name, args)
    msg = _slot(lib)
    assert msg.startswith(name.encode() + b": "), msg
    for w in words:
        assert w in msg[len(name) + 2:], (w, msg)
    return True


def test_every_satrl_refusal_names_its_entry_point():
    """Every satrl_* symbol of _lib._SIGS (one added later included), called
    with all-zero / NULL arguments, returns a negative code and leaves
    "<symbol>: <reason>" in the shared slot, which held another entry point's
    text before the call.  Nothing on these paths reaches a device."""
    import satrl._lib as L
    lib = L.lib()

    def zero(t):
        return None if t is C.c_void_p or issubclass(t, C._Pointer) else t(0).value

    # the whole exception list: each has its own case below
    special = {"satrl_last_error", "satrl_ppo_last_error", "satrl_span_probe", "satrl_span_probe_launches",
               "satrl_ppo_rowpass_sync", "satrl_ppo_rowpass_fault_inject"}
    names = [n for n in L.exported_symbols() if n.startswith("satrl_")]
    assert special <= set(names) and len(names) > 50
    for name in names:
        if name in special:
            continue
        argt, _ = L._SIGS[name]
        _poison(lib, name)
        rc = getattr(lib, name)(*[zero(t) for t in argt])
        assert rc < 0, (name, rc)
        assert _slot(lib).startswith(name.encode() + b": "), (name, _slot(lib))
    # the two accessors return the one slot (_slot compares them)
    _poison(lib, "satrl_last_error")
    # zeros are valid here: no probe buffer, and no launch logged in a process without one
    assert lib.satrl_span_probe(None, 0, None) == 0 and lib.satrl_span_probe_launches() == 0
    assert _refused(lib, "satrl_span_probe", None, 8, None, words=(b"bytes",))
    # modes 0 and 1 flip a process-wide switch, so only the refused mode is called
    assert _refused(lib, "satrl_ppo_rowpass_sync", 2, words=(b"mode",))
    assert _refused(lib, "satrl_ppo_rowpass_fault_inject", -1, 0, None, words=(b"group",))


def test_check_reports_the_failing_entry_point():
    """_lib.check raises with the refused call's own text, whichever source
    file the entry point lives in and whatever failed before it."""
    import satrl._lib as L
    lib = L.lib()
    fake = C.c_void_p(16)
    H, mb = 256, 4096
    kx = lib.satrl_ppo_kx_elems(H, mb)
    # two refusals of other entry points first: 16 splits into slabs for 8, and an empty scratch
    assert lib.satrl_ppo_dw2_kx(H, mb, -1, 16, fake, fake, kx, fake, 2 * 8 * H * H, None) == -1
    assert _slot(lib).startswith(b"satrl_ppo_dw2_kx: p2 holds")
    assert lib.satrl_moments_ordered(1000, fake, fake, fake, 0, None) == -1
    assert _slot(lib).startswith(b"satrl_moments_ordered: scratch holds 0 doubles")
    rc = lib.satrl_policy_act(256, 8, fake, fake, fake, 1.6, 0, 0, 0, None, fake, fake, None, None, None)
    with pytest.raises(L.NativeError, match=r"^satrl_policy_act failed \(-1\): satrl_policy_act: act1"):
        L.check(rc, "satrl_policy_act")
    assert lib.satrl_ppo_dw2_kx(H, mb, -1, 16, fake, fake, kx, fake, 2 * 8 * H * H, None) == -1
    rc = lib.satrl_ppo_rowpass(100, 64, -1, fake, None, fake, fake, 0.1, 0.01, 1.6, fake, fake, fake, fake, None)
    with pytest.raises(L.NativeError, match=r"^satrl_ppo_rowpass failed \(-1\): satrl_ppo_rowpass: H 100"):
        L.check(rc, "satrl_ppo_rowpass")
    # an entry point of the host build's source file writes the same slot
    rc = lib.satrl_scripted_act_host(2, fake, None, fake)
    with pytest.raises(L.NativeError, match=r"^satrl_scripted_act_host failed \(-1\): satrl_scripted_act_host: law"):
        L.check(rc, "satrl_scripted_act_host")
    # the env ABIs keep their own slots
    with pytest.raises(L.NativeError, match=r"satenv_cpu_num_envs failed \(-1\): satenv_cpu_num_envs"):
        L.check(lib.satenv_cpu_num_envs(None, None), "satenv_cpu_num_envs")
    with pytest.raises(L.NativeError, match=r"satenv_create failed \(-1\): satenv_create"):
        L.check(lib.satenv_create(None, 4, None, 0), "satenv_create")


def test_entry_points_reject_bad_arguments_before_any_device_call():
    """Error behaviour of the boundary (include/*.h: 0 ok, negative codes):
    shapes, widths and null pointers are checked on the host before any HIP
    call, so these run without a GPU.  A non-null dummy pointer is never
    dereferenced on these paths.  Every learner-side refusal names its entry
    point and says which check failed."""
    import ctypes as C
    import satrl._lib as L
    from satrl import env as E
    lib = L.lib()
    fake = C.c_void_p(16)                       # never touched: every call below fails its host checks

    def no(name, *args, words=()):
        return _refused(lib, name, *args, words=words)

    # satenv_create: null out / null params / num_envs <= 0 / bad propagator -> SATENV_ERR_ARG (-1)
    p = E.default_params()
    h = C.c_void_p()
    assert lib.satenv_create(None, 4, C.byref(p), 0) == -1
    assert lib.satenv_create(C.byref(h), 4, None, 0) == -1
    assert lib.satenv_create(C.byref(h), 0, C.byref(p), 0) == -1
    assert b"bad arguments" in lib.satenv_last_error()
    bad = E.default_params()
    bad.propagator = 7
    assert lib.satenv_create(C.byref(h), 4, C.byref(bad), 0) == -1
    assert b"propagator" in lib.satenv_last_error()
    assert lib.satenv_set_step_kernel(None, 2, 64) == -1 and lib.satenv_set_step_kernel(fake, 3, 64) == -1
    assert lib.satenv_set_step_kernel(fake, 2, 48) == -1                       # 16 / 32 / 64 envs per workgroup
    # learner side: unsupported hidden width, empty minibatch, net out of range, null buffers
    off = (C.c_int64 * 16)()
    assert no("satrl_ppo_layout", 100, off, words=(b"H 100",)) and lib.satrl_ppo_layout(256, off) == 0
    assert no("satrl_ppo_sizes", 256, 0, None, None, words=(b"mb 0",))
    args = [fake, None, fake, fake, 0.1, 0.01, 1.6, fake, fake, fake, fake, None]
    assert no("satrl_ppo_rowpass", 100, 64, -1, *args, words=(b"H 100", b"64/128/256"))   # H not 64/128/256
    assert no("satrl_ppo_rowpass", 256, 0, -1, *args, words=(b"mb 0", b"empty"))          # empty minibatch
    assert no("satrl_ppo_rowpass", 256, 64, 2, *args, words=(b"net 2", b"-1 .. 1"))       # net not -1/0/1
    assert no("satrl_ppo_rowpass", 256, 64, -1, None, *args[1:], words=(b"src is NULL",))  # null rows
    big = 1 << 40                                # a p2 / plane capacity no call exceeds
    assert no("satrl_ppo_dw2", 256, 4096, -1, 0, fake, fake, fake, big, None, words=(b"S 0 < 1",))      # S < 1
    assert no("satrl_ppo_dw2", 256, 64, -1, 64, fake, fake, fake, big, None,
              words=(b"empty split", b"satrl_ppo_dw2_splits"))                                          # an empty split
    assert no("satrl_ppo_reduce", 256, 64, -1, 1, 4, fake, big, fake, fake, fake, fake, fake, None,
              words=(b"mode",))                                                                         # mode
    assert no("satrl_ppo_reduce", 256, 64, -1, 1, 2, fake, big, fake, fake, fake, None, None, None,
              words=(b"nsq is NULL",))                                                                  # no nsq
    assert no("satrl_gae", 0, 4, fake, fake, fake, 0.99, 0.95, fake, fake, None, words=(b"T must",))
    assert no("satrl_gae", 4, 4, fake, None, fake, 0.99, 0.95, fake, fake, None, words=(b"done is NULL",))
    assert no("satrl_policy_act", 256, 8, fake, fake, fake, 1.6, 0, 0, 0, None, fake, fake, None, None, None,
              words=(b"act1 is NULL",))                                       # second agent without outputs
    assert no("satrl_ppo_tanh", 0, fake, fake, None, words=(b"n 0",))
    # the fc2 operand image and the k-packed dW2 path (H = 256, mb above the 16-row threshold)
    assert lib.satrl_ppo_w2x_floats(256) == 2 * 256 * 256                    # the f32 W2^T at every width
    assert lib.satrl_ppo_w2x_floats(64) == 2 * 64 * 64
    assert no("satrl_ppo_w2x_floats", 100, words=(b"H 100",))
    assert no("satrl_ppo_w2x_sync", 100, -1, fake, fake, None, words=(b"H 100",))
    assert no("satrl_ppo_w2x_sync", 256, -1, None, fake, None, words=(b"P is NULL",))
    assert lib.satrl_ppo_kx_elems(256, 4096) == 2 * 3 * 4096 * 256 and lib.satrl_ppo_kx_elems(256, 1500) == 6 * 1504 * 256
    assert no("satrl_ppo_kx_elems", 64, 4096, words=(b"H 64 is not 256",))
    kx_args = args[:9] + [big] + args[9:]        # (H1x, dZ2x, kx_elems, ptail, pw1, stream)
    assert no("satrl_ppo_rowpass_kx", 256, 512, -1, None, *kx_args[1:],
              words=(b"src is NULL",))                                        # null rows (16-row kernel's minibatch)
    assert no("satrl_ppo_rowpass_kx", 64, 4096, -1, *kx_args, words=(b"H 64 is not 256",))   # H 256 only
    assert lib.satrl_ppo_dw2_kx_splits(256, 4096, -1) == 8 and lib.satrl_ppo_dw2_kx_splits(256, 4096, 0) == 16
    assert no("satrl_ppo_dw2_kx", 256, 4096, -1, 0, fake, fake, big, fake, big, None, words=(b"S 0 < 1",))   # S < 1
    assert no("satrl_ppo_dw2_kx", 256, 64, -1, 3, fake, fake, big, fake, big, None,
              words=(b"empty split", b"satrl_ppo_dw2_kx_splits"))             # an empty split (2 chunks)
    assert no("satrl_ppo_dw2_kx", 256, 4096, -1, 8, None, fake, big, fake, big, None,
              words=(b"H1x is NULL",))                                        # null H1x
    w1a = [fake, fake, big, fake, big]                     # (H1x, dZ2x, kx_elems, p2, p2_floats)
    w1 = "satrl_ppo_dw2_kx_w1"
    assert no(w1, 256, 4096, -1, 8, *w1a, 2, fake, fake, fake, fake, None, words=(b"mode 2", b"1 or 3"))  # mode 1 or 3
    assert no(w1, 256, 4096, -1, 8, *w1a, 3, None, fake, fake, fake, None, words=(b"p1 is NULL",))       # null p1
    assert no(w1, 256, 4096, -1, 8, *w1a, 3, fake, fake, fake, None, None, words=(b"nsq", b"mode 3"))    # mode 3: nsq
    assert no(w1, 64, 4096, -1, 8, *w1a, 1, fake, fake, fake, None, None, words=(b"H 64 is not 256",))   # H 256 only
    assert no("satrl_ppo_reduce", 256, 4096, -1, 8, 6, fake, big, None, None, fake, fake, fake, None,
              words=(b"bit 4", b"without 1"))                                 # 4 needs 1
    assert no("satrl_ppo_rowpass_error", None, 1.0, None, words=(b"err is NULL",))   # the column-split kernel's error word
    assert no("satrl_ppo_rowpass_error", C.byref(C.c_int()), 0.0, None, words=(b"deadline",))   # no deadline
    assert no("satrl_ppo_rowpass_fault_inject", -1, 0, None, words=(b"group -1",))
    assert no("satrl_ppo_rowpass_fault_inject", 1 << 20, 0, None, words=(b"group 1048576",))
    # the peer all-reduce: grid, deadline, buffers
    bufs = (C.c_void_p * 2)(16, 16)
    pa = [C.cast(bufs, C.c_void_p), fake, fake, fake]
    ar = "satrl_ppo_allreduce_peer"
    assert no(ar, 256, 512, 2, 0, *pa, 0, 10.0, None, words=(b"blocks 0",))                  # no blocks
    assert no(ar, 256, 512, 2, 0, *pa, 2048, 10.0, None, words=(b"blocks 2048", b"1024"))    # > kPeerMaxBlocks
    assert no(ar, 256, 512, 2, 0, *pa, 256, 0.0, None, words=(b"deadline",))                 # no deadline
    assert no(ar, 256, 512, 2, 2, *pa, 256, 10.0, None, words=(b"rank 2", b"0 .. 1"))        # rank >= world
    assert no(ar, 256, 512, 9, 0, *pa, 256, 10.0, None, words=(b"world 9", b"8"))            # world > 8
    assert no("satrl_peer_blocks", 100, C.byref(C.c_int()), words=(b"H 100",))
    assert no("satrl_peer_blocks", 256, None, words=(b"blocks is NULL",))
    assert no("satrl_peer_error", None, C.byref(C.c_uint64()), None, words=(b"buf is NULL",))
    assert no("satrl_peer_reset", fake, 8, None, words=(b"header",))                         # smaller than the header


def test_capi_refuses_calls_past_the_callers_buffers():
    """Round-5 fault (a dW2 run with more splits than its slabs were sized
    for wrote past p2): every call that writes or reads the dW2 slabs or the
    k-packed planes takes the caller's capacity and refuses with -1 before
    any launch (fake pointers, never touched; a launch would fail with -2 on
    this GPU-less host instead)."""
    import ctypes as C
    import satrl._lib as L
    lib = L.lib()
    fake = C.c_void_p(16)
    H, mb = 256, 4096
    S = lib.satrl_ppo_dw2_kx_splits(H, mb, -1)                    # 8
    kx = lib.satrl_ppo_kx_elems(H, mb)
    p2_8 = 2 * 8 * H * H                                         # slabs sized for 8 splits
    # an oversize split count (the round-5 case: 16 splits into slabs for 8)
    def no(name, *args, words):
        return _refused(lib, name, *args, words=words)

    assert no("satrl_ppo_dw2_kx", H, mb, -1, 16, fake, fake, kx, fake, p2_8, None, words=(b"p2 holds", b"16 splits"))
    assert b"p2 holds" in lib.satrl_ppo_last_error()
    assert no("satrl_ppo_reduce", H, mb, -1, 16, 3, fake, p2_8, fake, fake, fake, fake, fake, None,
              words=(b"p2 holds", b"16 splits"))
    assert b"p2 holds" in lib.satrl_ppo_last_error()
    assert no("satrl_ppo_dw2", H, mb, -1, 16, fake, fake, fake, p2_8, None, words=(b"p2 holds", b"16 splits"))
    # one net: the actor passes half, the critic (second half) the whole buffer
    assert no("satrl_ppo_dw2_kx", H, mb, 1, S, fake, fake, kx, fake, p2_8 // 2, None, words=(b"p2 holds",))
    # undersized planes, for the rowpass that writes them and the dW2 that reads them
    assert no("satrl_ppo_rowpass_kx", H, mb, -1, fake, None, fake, fake, 0.1, 0.01, 1.6, fake, fake, kx - 1, fake,
              fake, None, words=(b"planes hold",))
    assert b"planes hold" in lib.satrl_ppo_last_error()
    assert no("satrl_ppo_dw2_kx", H, mb, -1, S, fake, fake, kx - 1, fake, p2_8, None, words=(b"planes hold",))
    # H 64: one slab per 32-row block (128 at mb 4096) written by the fused rowpass
    assert no("satrl_ppo_rowpass_dw2", 64, mb, -1, fake, None, fake, fake, 0.1, 0.01, 1.6, fake, 2 * 127 * 64 * 64,
              fake, fake, None, words=(b"p2 holds", b"128 splits"))
    assert b"p2 holds" in lib.satrl_ppo_last_error()


def test_product_has_no_cpu_fallback():
    import torch
    from satrl import env as E
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(Exception):
        E.VecSatellites(4)


def test_reference_module_name_shims():
    """`from environment import satellites` etc. (CPPO_main.py:5-7) resolve to the engine."""
    import importlib
    import sys
    from conftest import PKG_DIR
    sys.path.insert(0, str(PKG_DIR))
    try:
        env = importlib.import_module("environment")
        ppo = importlib.import_module("ppo_continuous")
        rb = importlib.import_module("replaybuffer")
        main = importlib.import_module("CPPO_main")
    finally:
        sys.path.remove(str(PKG_DIR))
    import satrl.buffer
    import satrl.env
    import satrl.ppo
    import satrl.trainer
    assert env.satellites is satrl.env.satellites
    assert ppo.PPO_continuous is satrl.ppo.PPO_continuous
    assert rb.ReplayBuffer is satrl.buffer.ReplayBuffer
    assert main.args_param is satrl.trainer.args_param
    assert main.train_pursuer_network is satrl.trainer.train_pursuer_network


def test_improvednn_matches_reference_state_dict(tmp_path):
    """satrl.surrogate.ImprovedNN has the reference's parameter names/shapes:
    the MLPNet2.pth state_dict (single_pluse_model/; its tensors are kept
    under their own names in tests/golden/mlpnet2.npz), saved as a .pth file,
    loads with weights_only=True and strict key matching, and the net then
    gives the outputs the reference's net gave for the stored inputs."""
    import numpy as np
    import torch
    from conftest import golden
    from satrl.surrogate import ImprovedNN
    g = golden("mlpnet2")
    names = [k for k in g.files if k.endswith((".weight", ".bias"))]
    assert names == [f"fc{i}.{p}" for i in (1, 2, 3, 4) for p in ("weight", "bias")]
    path = str(tmp_path / "MLPNet2.pth")
    torch.save({k: torch.from_numpy(g[k]) for k in names}, path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    net = ImprovedNN()
    net.load_state_dict(sd)
    net.eval()
    with torch.no_grad():
        out = net(torch.zeros(1, 5))
        y = net(torch.from_numpy(g["x"])).numpy()
    assert out.shape == (1, 10) and torch.isfinite(out).all()
    # the same f32 torch-CPU forward as the capture: round-off of the GEMM blocking only
    assert np.allclose(y, g["y"], rtol=1e-4, atol=1e-5 * float(np.abs(g["y"]).max()))


def test_w2x_image_host_statement():
    """The fc2 operand image's host statement (satrl.ppo.w2x_image, what
    satrl_ppo_w2x_sync writes): the f32 fc2.weight^T of both nets at every
    width, and w2x_decode recovers it bit for bit."""
    import torch
    from satrl.ppo import w2x_decode, w2x_image
    g = torch.Generator().manual_seed(0)
    for H in (64, 256):
        W2 = torch.randn(2 * H * H, generator=g) * torch.exp(torch.randn(2 * H * H, generator=g) * 4)
        img = w2x_image(W2, H)
        assert img.dtype == torch.float32 and img.numel() == 2 * H * H
        assert torch.equal(w2x_decode(img, H), W2.view(2, H, H).transpose(1, 2))


def test_uses_column_split():
    """Which updates need the exchange check (ppo_kernels.hip cs_fits: H 256,
    a minibatch or ragged tail of at most 1024 rows)."""
    from satrl.ppo import uses_column_split
    assert uses_column_split(256, 512, 8192) and uses_column_split(256, 1024, 8192)
    assert not uses_column_split(256, 4096, 8192)            # configs[1]-sized minibatches, no tail
    assert uses_column_split(256, 4096, 8192 + 100)           # a 100-row tail
    assert not uses_column_split(256, 4096, 8192 + 2000)      # a tail over 1024 rows
    assert uses_column_split(256, 4096, 700)                  # one minibatch of the whole 700 rows
    assert not uses_column_split(64, 512, 8192) and not uses_column_split(128, 512, 8192)
