"""The two synchronisation forms of the 32-row 16-wave H 256 k-packed rowpass
(ppo_kernels.hip RpBarrier / RpHandoff, selected by satrl_ppo_rowpass_sync):
the per-chunk LDS hand-offs must give every output bit of the workgroup
barriers, which are the oracle here (the barrier form is checked against
torch and the f32 rowpass by test_ppo_gpu.py).

Shapes, both nets in one launch, through satrl_ppo_rowpass_kx32 (the 32-row
kernel at any size; the product sends minibatches up to 1024 rows to the
16-row kernels): one full block (32 rows); one block and a ragged one whose
valid rows end in its first 16-row tile (40) and in its second (55); 8 row
blocks (256: the XCD-matched block placement) and 9 (288: the other one).
Then a captured graph of minibatch steps replayed in each form: the hand-off
words are re-initialised by every launch, and the error word stays zero.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 256


def _args(**kw):
    from satrl.trainer import args_param
    a = args_param(chkpt_dir="/tmp", **kw)
    a.state_dim, a.action_dim, a.max_action = 18, 3, 1.6
    return a


def _rows(B, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    src = torch.randn((B, 32), device="cuda", generator=g)
    src[:, 21:24] = -1.0 - torch.rand((B, 3), device="cuda", generator=g)
    return src, g


@pytest.fixture()
def sync_switch():
    """Sets the process-wide form; the previous one comes back afterwards."""
    from satrl.ppo import rowpass_sync
    prev = rowpass_sync()
    yield rowpass_sync
    rowpass_sync(prev)


@pytest.fixture(scope="module")
def learner():
    from satrl.ppo import PPOLearner
    torch.manual_seed(5)
    L = PPOLearner(_args(hidden_width=H, mini_batch_size=288, batch_size=2048), "pursuer", use_graph=False)
    with torch.no_grad():
        for p in list(L.actor.parameters()) + list(L.critic.parameters()):
            p.add_(torch.randn_like(p) * 0.05)
    L.sync_w2t()
    return L


def _rowpass32(L, st, src, idx, mb, ratio):
    import satrl._lib as _L
    from satrl._lib import check, ptr
    check(_L.lib().satrl_ppo_rowpass_kx32(H, mb, -1, ptr(src), None if idx is None else ptr(idx), ptr(L.P), ptr(L.W2T),
                                          float(L.epsilon), float(L.entropy_coef), float(L.max_action), ptr(st.H1x),
                                          ptr(st.dZ2x), st.H1x.numel(), ptr(st.ptail), ptr(st.pw1), ptr(ratio),
                                          _L.stream_ptr()), "satrl_ppo_rowpass_kx32")


@pytest.mark.parametrize("mb,contig", [(32, True), (40, True), (55, False), (256, True), (288, False)])
def test_handoff_rowpass_is_bitwise_the_barrier_rowpass(learner, sync_switch, mb, contig):
    """Every output of one launch: the H1 and dZ2 planes (the whole padded
    buffers), the [dW1|db1] slabs, the tail slabs and the actor's ratio."""
    from satrl.ppo import rowpass_exchange_check
    L = learner
    src, g = _rows(2048, 6)
    idx = None if contig else torch.randperm(2048, device="cuda", generator=g)[:mb]
    st = L.stepper(mb)
    assert st.kx(mb)
    rowpass_exchange_check()
    outs = []
    for mode in (0, 1):
        sync_switch(mode)
        # (slots the launch never writes: the same finite bytes in both runs)
        st.H1x.fill_(-1)
        st.dZ2x.fill_(-1)
        st.ptail.fill_(7.0)
        st.pw1.fill_(7.0)
        ratio = torch.full((mb,), 7.0, device="cuda")
        _rowpass32(L, st, src, idx, mb, ratio)
        torch.cuda.synchronize()
        outs.append([t.clone() for t in (st.H1x, st.dZ2x, st.pw1, st.ptail, ratio)])
    rowpass_exchange_check()                       # no hand-off wait ran out
    bar, hoff = outs
    rows = (mb + 31) // 32 * 32
    # the barrier form did write what is compared: planes of the padded rows, a ratio per row, slabs per block
    assert not (bar[0][:6 * rows * H] == -1).all() and not (bar[1][:6 * rows * H] == -1).all()
    assert (bar[4] != 7.0).all() and (bar[2][:rows // 32 * 2 * H * 20] != 7.0).any()
    for name, a, b in zip(("H1 planes", "dZ2 planes", "[dW1|db1] slabs", "tail slabs", "ratio"), bar, hoff):
        assert torch.equal(a, b), name


def test_handoff_rowpass_in_a_replayed_graph(sync_switch):
    """Two epochs of graph-replayed minibatch steps (1056 rows: 33 row blocks
    of the 32-row kernel, groups of 2 steps per graph, 3 replays per epoch) in
    the hand-off form leave bitwise the parameters, Adam moments and step
    counters of the barrier form, and the error word stays zero: the hand-off
    words start from zero in every launch of a replay."""
    from satrl.ppo import PPOLearner, rowpass_exchange_check
    mb, G = 1056, 2
    B = 3 * G * mb
    rowpass_exchange_check()
    res = []
    for mode in (0, 1):
        sync_switch(mode)                           # before the capture: a graph keeps its form
        torch.manual_seed(11)
        L = PPOLearner(_args(hidden_width=H, mini_batch_size=mb, batch_size=B), "pursuer", graph_group=G,
                       use_graph=True)
        src, g = _rows(B, 2)
        perms = [torch.randperm(B, device="cuda", generator=g) for _ in range(2)]
        L.sync_w2t()
        st = L.stepper(mb)
        P0 = L.P.clone()
        for p in perms:
            st.run(src, p)
        torch.cuda.synchronize()
        assert st.graph is not None and int(st.grp.item()) == 3
        assert not torch.equal(L.P, P0)             # the steps were taken
        res.append((L.P.clone(), L.M.clone(), L.V.clone(), L.steps.clone()))
    rowpass_exchange_check()
    for a, b in zip(*res):
        assert torch.equal(a, b)
