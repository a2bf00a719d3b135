"""`BatchedAdam.step` on the GPU (csrc/k_adam.hip) against the float64 restatement and the bars of tests/optim_ref.py:
norms within 4 u, m / v / param within their bars with the coefficient formed from the PUBLISHED norm, `step_torch` on the
device within the same bars; every tensor a view inside a buffer of NaN-bit sentinels that must stay bitwise unchanged.
C = the elements one workgroup handles."""
import pytest
import torch

from ris_vec_marl_amd import BatchedAdam, BatchedCritic, BatchedLocalCritics, BatchedTwinCritic
from ris_vec_marl_amd import _native as N
from ris_vec_marl_amd._weights import soft_update_tensors
from tests import optim_ref as R

pytestmark = pytest.mark.gpu
C = N.ADAM_CHUNK
SIZES = (1, 3, 4, 5, C - 1, C, C + 1, 3 * C - 1)
SENTINEL = 0x7FC0DEAD


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


class Views:
    """Tensors as views inside sentinel buffers, `off` floats past a 16-byte boundary."""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def new(self, data: torch.Tensor, off: int = 0) -> torch.Tensor:
        n = data.numel()
        buf = torch.full((n + 24,), SENTINEL, dtype=torch.int32, device=self.dev)
        assert buf.data_ptr() % 16 == 0
        view = buf.view(torch.float32)[8 + off:8 + off + n]
        view.copy_(data.reshape(-1))
        self.bufs.append((buf, 8 + off, n))
        return view

    def intact(self) -> bool:
        return all(bool((b[:lo] == SENTINEL).all()) and bool((b[lo + n:] == SENTINEL).all()) for b, lo, n in self.bufs)


def build(dev, sizes_per_group, seed=0, offs=(0, 0, 0), grad=None, targets=True, post=None):
    """-> (views, params, grads, targets): nested lists; grad(n, generator, group, k) draws a gradient, post(P, G, T) edits
    the tensors in place afterwards."""
    g = torch.Generator().manual_seed(seed)
    vw = Views(dev)
    P, G, T = [], [], []
    for gi, sizes in enumerate(sizes_per_group):
        P.append([vw.new(torch.randn(n, generator=g), offs[0]) for n in sizes])
        G.append([vw.new(grad(n, g, gi, k) if grad else torch.randn(n, generator=g), offs[1]) for k, n in enumerate(sizes)])
        T.append([vw.new(torch.randn(n, generator=g), offs[2]) for n in sizes] if targets else None)
    if post:
        post(P, G, T)
    return vw, P, G, (T if targets else None)


def snapshot(opt):
    i, out = 0, []
    for grp in opt.groups:
        out.append([(p.detach().cpu().clone(), opt.exp_avg[i + k].cpu().clone(), opt.exp_avg_sq[i + k].cpu().clone())
                    for k, p in enumerate(grp)])
        i += len(grp)
    return out


def judge(before, after, grads, norms, opt, t, check_norm=True):
    """after vs optim_ref from `before`; the coefficient of each group from the published norm.  -> worst ratios"""
    worst = {"m": 0.0, "v": 0.0, "p": 0.0, "norm_u": 0.0}
    for gi, (b, a, gs) in enumerate(zip(before, after, grads)):
        coef = 1.0
        if opt.max_norm[gi] is not None:
            want = R.norm_ref(gs)
            if check_norm and want > 0:
                worst["norm_u"] = max(worst["norm_u"], abs(float(norms[gi].double()) - want) / (R.U32 * want))
            elif check_norm:
                assert float(norms[gi]) == 0.0
            coef = R.coef_f32(norms[gi].cpu(), opt.max_norm[gi])
        for (p, m, v), (p1, m1, v1), g in zip(b, a, gs):
            ref = R.adam_ref(p, g, m, v, coef, opt.lr[gi], opt.betas, opt.eps, opt.weight_decay[gi], t)
            for k, got in (("m", m1), ("v", v1), ("p", p1)):
                worst[k] = max(worst[k], R.worst_ratio(got, ref[k], ref[k + "_bar"]))
    print("|err| / bar", worst)
    assert worst["m"] <= 1 and worst["v"] <= 1 and worst["p"] <= 1 and worst["norm_u"] <= R.NORM_K
    return worst


def run_and_judge(dev, sizes_per_group, t0=0, offs=(0, 0, 0), grad=None, seed=0, post=None, **hyper):
    """One `step` and one `step_torch` from equal states, both judged; sentinels and gradients checked."""
    hyper.setdefault("max_norm", 1.0)
    out = []
    for method in ("step", "step_torch"):
        vw, P, G, T = build(dev, sizes_per_group, seed, offs, grad, post=post)
        opt = BatchedAdam(P, **hyper)
        if t0:
            g = torch.Generator().manual_seed(seed + 99)
            sd = opt.state_dict()
            sd["step"] = t0
            sd["exp_avg"] = [[torch.randn(p.shape, generator=g) * 0.1 for p in grp] for grp in P]
            sd["exp_avg_sq"] = [[torch.randn(p.shape, generator=g) ** 2 * 0.01 for p in grp] for grp in P]
            opt.load_state_dict(sd)
        before, g_before = snapshot(opt), [[x.clone() for x in grp] for grp in G]
        t_before = [[x.clone() for x in grp] for grp in T]
        norms = getattr(opt, method)(targets=T, tau=0.005, grads=G)
        torch.cuda.synchronize()
        assert opt.t == t0 + 1 and vw.intact()
        assert all(torch.equal(a, b) for ga, gb in zip(G, g_before) for a, b in zip(ga, gb))       # write-back is off
        judge(before, snapshot(opt), [[x.cpu() for x in grp] for grp in G], norms, opt, t0 + 1, check_norm=method == "step")
        for grp, tg, tb in zip(P, T, t_before):
            for p, t, b in zip(grp, tg, tb):
                assert torch.equal(t, 0.005 * p + (1 - 0.005) * b)                                # the reference's statement
        out.append((opt, P, T, norms))
    return out


# ---------------------------------------------------------------------- sizes, alignment, groups
OFFS = [(0, 0, 0)] + [tuple(o if i == k else 0 for i in range(3)) for k in range(3) for o in (1, 2, 3)] + [(o, o, o) for o in (1, 2, 3)]


@pytest.mark.parametrize("offs", OFFS)
def test_every_size_at_every_offset_from_a_16_byte_boundary(dev, offs):
    (opt, _, _, _), _ = run_and_judge(dev, [SIZES], offs=offs)
    assert opt.n_blocks == sum((n + C - 1) // C for n in SIZES)


@pytest.mark.parametrize("n_groups", [1, 2, 33])
def test_group_counts(dev, n_groups):
    small = (1, 3, 4, 5, 17, 64, 255, 1023)
    if n_groups == 2:
        sizes = [SIZES, (1,)]                                 # the second group is a lone one-element tensor
    else:
        sizes = [SIZES if gi == 0 else tuple(s + gi for s in small) for gi in range(n_groups)]
    lr = [1e-3 * (1 + gi % 3) for gi in range(len(sizes))]
    (opt, _, _, norms), _ = run_and_judge(dev, sizes, lr=lr, seed=n_groups)
    assert norms.shape == (len(sizes),) and len(opt._params) == sum(len(s) for s in sizes)
    if n_groups == 33:
        assert len(opt._params) == 264


# ---------------------------------------------------------------------- gradients
def _to_norm(norm):
    """Rescale every group's gradients to this norm (formed in float64; the float32 products move it by ~1e-7)."""
    def post(P, G, T):
        for grp in G:
            scale = norm / R.norm_ref(grp)
            for x in grp:
                x.mul_(scale)
    return post


def _mixed(n, g, gi, k):
    return torch.randn(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * 15 - 12)


@pytest.mark.parametrize("name", ["zero", "under", "far_over", "mixed", "mixed_unclipped"])
def test_gradient_magnitudes(dev, name):
    grad = {"zero": lambda n, g, gi, k: torch.zeros(n), "mixed": _mixed, "mixed_unclipped": _mixed}.get(name)
    post = {"under": _to_norm(0.9999), "far_over": _to_norm(1e4)}.get(name)
    hyper = {"max_norm": 1e6} if name == "mixed_unclipped" else {}      # 1e-12 .. 1e3 reach the moments as they are
    (opt, P, _, norms), _ = run_and_judge(dev, [SIZES, SIZES[:4]], grad=grad, post=post, seed=3, **hyper)
    n0 = float(norms[0])
    if name == "zero":
        assert n0 == 0.0
    elif name == "under":
        assert 0.9998 < n0 < 1.0 and R.coef_f32(norms[0].cpu(), 1.0) == 1.0     # clamped to 1
    elif name == "far_over":
        assert 0.9999e4 < n0 < 1.0001e4
    elif name == "mixed_unclipped":
        assert R.coef_f32(norms[0].cpu(), 1e6) == 1.0


def test_a_nonfinite_gradient_takes_its_group_only(dev):
    for method in ("step", "step_torch"):
        vw, P, G, T = build(dev, [SIZES[:5], SIZES, SIZES[:4]], seed=5)
        G[1][5][17] = float("nan")
        opt = BatchedAdam(P)
        norms = getattr(opt, method)(grads=G)
        torch.cuda.synchronize()
        assert vw.intact()
        assert torch.isnan(norms[1]) and torch.isfinite(norms[0]) and torch.isfinite(norms[2])
        assert all(bool(torch.isnan(p).all()) for p in P[1])
        if method == "step":
            for gi in (0, 2):                                 # the other groups are exactly what they are without group 1
                _, P2, G2, _ = build(dev, [SIZES[:5], SIZES, SIZES[:4]], seed=5)
                alone = BatchedAdam([P2[gi]])
                alone.step(grads=[G2[gi]])
                assert all(torch.equal(a, b) for a, b in zip(P[gi], P2[gi]))
        assert all(bool(torch.isfinite(p).all()) for gi in (0, 2) for p in P[gi])


# ---------------------------------------------------------------------- steps and options
@pytest.mark.parametrize("t0", [0, 1, 999])
def test_step_counts_through_load_state_dict(dev, t0):
    run_and_judge(dev, [SIZES[3:7], SIZES[:3]], t0=t0, seed=t0, lr=[1e-3, 3e-4])


def test_weight_decay_and_per_group_lr(dev):
    run_and_judge(dev, [SIZES, SIZES[:4]], t0=1, weight_decay=0.01, lr=[1e-3, 3e-4], seed=11)
    run_and_judge(dev, [SIZES[:6], SIZES[:4]], weight_decay=[0.0, 0.01], max_norm=[None, 0.5], seed=12)


def test_without_clipping_it_is_one_launch(dev):
    vw, P, G, T = build(dev, [SIZES, SIZES[:4]], seed=13)
    opt = BatchedAdam(P, max_norm=None, weight_decay=0.01)
    before = snapshot(opt)
    assert opt.step(targets=T, tau=0.005, grads=G) is None
    assert N.last_kernel() == "k_adam_step"
    judge(before, snapshot(opt), [[x.cpu() for x in grp] for grp in G], None, opt, 1)
    assert vw.intact()
    clip = BatchedAdam(build(dev, [SIZES[:3]], seed=1)[1])
    clip.step(grads=[[torch.ones_like(p) for p in clip.groups[0]]])
    assert N.last_kernel() == "k_adam_sqsum + k_adam_step"


def test_write_back_gives_grad_times_coef_bit_for_bit(dev):
    vw, P, G, _ = build(dev, [SIZES, SIZES[:4]], seed=14, offs=(0, 1, 0), post=_to_norm(30.0), targets=False)
    g0 = [[x.clone() for x in grp] for grp in G]
    opt = BatchedAdam(P, write_clipped_grads=True)
    before = snapshot(opt)
    norms = opt.step(grads=G)
    judge(before, snapshot(opt), [[x.cpu() for x in grp] for grp in g0], norms, opt, 1)
    for gi in range(2):
        coef = torch.clamp(1.0 / (norms[gi] + 1e-6), max=1.0)
        assert float(coef) < 1.0
        assert all(torch.equal(x, x0 * coef) for x, x0 in zip(G[gi], g0[gi]))
    assert vw.intact()


# ---------------------------------------------------------------------- blend, determinism, pointers
@pytest.mark.parametrize("tau", [0.005, 1.0])
def test_blend_in_the_same_pass_is_step_then_soft_update_bit_for_bit(dev, tau):
    outs = []
    for fused in (True, False):
        vw, P, G, T = build(dev, [SIZES, SIZES[:4]], seed=15, offs=(0, 0, 2))
        opt = BatchedAdam(P)
        if fused:
            opt.step(targets=T, tau=tau, grads=G)
        else:
            opt.step(grads=G)
            soft_update_tensors([(p, t) for gp, gt in zip(P, T) for p, t in zip(gp, gt)], tau, dev)
        outs.append([x.clone() for grp in P + T for x in grp] + [x.clone() for x in opt.exp_avg + opt.exp_avg_sq])
        assert vw.intact()
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    if tau == 1.0:
        assert all(torch.equal(a, b) for a, b in zip(outs[0][:12], outs[0][12:24]))      # a hard copy


def test_two_fresh_optimisers_agree_bit_for_bit_and_every_workgroup_has_one_coefficient(dev):
    def const(n, g, gi, k):
        return torch.full((n,), 0.37) if n == 3 * C - 1 else torch.randn(n, generator=g)
    runs = []
    for _ in range(2):
        vw, P, G, T = build(dev, [SIZES, SIZES[:4]], seed=16, grad=const)
        P[0][7].fill_(1.25)
        opt = BatchedAdam(P, lr=1e-2)
        got = []
        for s in range(3):
            norms = opt.step(targets=T, tau=0.005, grads=G)
            got += [norms.clone()] + [x.clone() for grp in P + T for x in grp] + [x.clone() for x in opt.exp_avg + opt.exp_avg_sq]
            assert P[0][7].unique().numel() == 1 and float(P[0][7][0]) != 1.25     # three workgroups, one value
        runs.append(got)
        assert float(norms[0]) > 1.0 and vw.intact()                                # the coefficient is not the clamp's 1
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_moved_gradients_are_followed_and_the_table_is_sent_only_then(dev):
    vw, P, G, T = build(dev, [SIZES[:6], SIZES[:4]], seed=17)
    P = [[p.requires_grad_() for p in grp] for grp in P]
    opt = BatchedAdam(P)
    for grp, gg in zip(P, G):
        for p, g in zip(grp, gg):
            p.grad = g
    opt.step(targets=T, tau=0.005)
    opt.step(targets=T, tau=0.005)
    assert opt.table_uploads == 1
    keep = [x.clone() for grp in G for x in grp]              # hold the old gradients so that the new ones are elsewhere
    v0 = [p._version for grp in P for p in grp]
    g = torch.Generator().manual_seed(18)
    fresh = []
    for grp in P:                                             # zero_grad(set_to_none=True), then a backward's new tensors
        for p in grp:
            p.grad = None
        fresh.append([torch.randn(p.shape, generator=g).to(dev) for p in grp])
        for p, x in zip(grp, fresh[-1]):
            p.grad = x
    before = snapshot(opt)
    norms = opt.step(targets=T, tau=0.005)
    assert opt.table_uploads == 2 and opt.t == 3
    judge(before, snapshot(opt), [[x.cpu() for x in grp] for grp in fresh], norms, opt, 3)
    assert all(p._version > v for p, v in zip([p for grp in P for p in grp], v0))
    opt.step(targets=T, tau=0.005)
    assert opt.table_uploads == 2
    opt.step()                                                # no targets: other pointers
    assert opt.table_uploads == 3 and vw.intact() and len(keep) == 10


# ---------------------------------------------------------------------- with the critic classes
def test_a_twin_critic_sharing_the_parameters_rebuilds_once_per_step(dev):
    S, A, n = 40, 80, 64
    g = torch.Generator().manual_seed(19)
    critic = BatchedTwinCritic(S, A, device=dev, seed=1)
    target = BatchedTwinCritic(S, A, device=dev, seed=2)
    critic.pack = target.pack = "device"
    groups = [[getattr(net, a) for a in net._WEIGHTS] for net in critic.nets]
    grads = [[(torch.randn(p.shape, generator=g) * 1e-2).to(dev) for p in grp] for grp in groups]
    state, action = torch.randn(n, S, generator=g).to(dev), torch.randn(n, A, generator=g).to(dev)
    reward, done = torch.randn(n, generator=g).to(dev), (torch.rand(n, generator=g) < 0.1).to(dev)
    critic.forward(state, action)
    target.td_target(reward, state, action, done)
    opt = BatchedAdam(groups, lr=1e-2)
    for s in range(2):
        packs, tpacks = critic.packs, target.packs
        versions = [p._version for grp in groups for p in grp]
        opt.step(targets=target, tau=0.005, grads=grads)
        assert all(p._version == v + 1 for p, v in zip([p for grp in groups for p in grp], versions))
        q = critic.forward(state, action)
        y = target.td_target(reward, state, action, done)
        assert critic.packs == packs + 2 and target.packs == tpacks + 2            # one rebuild per net and step
        critic.forward(state, action)
        assert critic.packs == packs + 2
        fresh = BatchedTwinCritic(S, A, device=dev, seed=3)
        fresh.load_state_dict(*critic.state_dict())
        assert all(torch.equal(a, b) for a, b in zip(q, fresh.forward(state, action)))
        fresh.load_state_dict(*target.state_dict())
        assert torch.equal(y, fresh.td_target(reward, state, action, done))


# ---------------------------------------------------------------------- driver sizes
def _driver_step(dev, groups, seed, **hyper):
    g = torch.Generator().manual_seed(seed)
    grads = [[(torch.randn(p.shape, generator=g) * 1e-2).to(dev) for p in grp] for grp in groups]
    opt = BatchedAdam(groups, **hyper)
    before = snapshot(opt)
    norms = opt.step(grads=grads)
    judge(before, snapshot(opt), [[x.cpu() for x in grp] for grp in grads], norms, opt, 1)
    return opt


def test_driver_size_global_twin_critics(dev):
    critic = BatchedTwinCritic(40, 80, 1024, 512, 256, device=dev, seed=4)
    opt = _driver_step(dev, [[getattr(net, a) for a in net._WEIGHTS] for net in critic.nets], 20, lr=3e-4)
    assert sum(p.numel() for p in opt._params) == 2 * (120 * 1024 + 1024 + 1024 * 512 + 512 + 512 * 256 + 256 + 256 + 1)


def test_driver_size_sixteen_local_critics(dev):
    local = BatchedLocalCritics(8, device=dev, seed=5)
    opt = _driver_step(dev, [[getattr(net, a) for a in net._WEIGHTS] for pair in local.nets for net in pair], 21, lr=3e-4)
    assert len(opt.groups) == 16 and len(opt._params) == 128


def test_driver_size_sarl_critic_with_decay_and_no_clip(dev):
    critic = BatchedCritic(80, 56, device=dev, seed=6)
    _driver_step(dev, [[getattr(critic, a) for a in critic._WEIGHTS]], 22, lr=1e-3, weight_decay=0.01, max_norm=None)
    assert N.last_kernel() == "k_adam_step"
