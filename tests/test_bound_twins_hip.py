"""The rollout stages behind their two doors: every unbound method (`store_batch`, `group`, ...) is the builder of its
`bind_*` twin called once, the input rule being the only difference -- `N.converted` (copied if needed) against
`N.in_place` (used as it is or refused).  Twins must leave identical bytes; bound launchers must refuse what they would
have to copy; unbound methods must take it and compute the same; and where the twins used to disagree the stricter
answer holds for both."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests.test_hip_parity import make_vec  # noqa: E402

DEV = "cuda:0"
KINDS = ("non-contiguous", "wrong dtype", "host")


def variant(x, kind):
    """`x` with the same values in a form a launcher cannot read in place."""
    if kind == "host":
        return x.cpu()
    if kind == "wrong dtype":
        return x.to(torch.int64 if x.dtype == torch.int32 else torch.float64)
    if x.dim() == 1:
        v = torch.stack([x, x], 1)[:, 0]
    else:
        v = x.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not v.is_contiguous() and torch.equal(v, x)
    return v


def rand(gen, *shape):
    return torch.rand(*shape, device=DEV, generator=gen) * 2 - 1


def ring_bytes(buf):
    return [getattr(buf, k).cpu().numpy().tobytes() for k in buf._ARRAYS] + [buf.mem_cntr]


def store_inputs(n, V, seed):
    gen = torch.Generator(device=DEV); gen.manual_seed(seed)
    return dict(state=rand(gen, n, V, 5), action=rand(gen, n, V * (V + 2)), metrics=rand(gen, n, 16), reward=rand(gen, n, V),
                state_=rand(gen, n, V, 5), mask=(rand(gen, n, V, V) < 0.2).to(torch.uint8), power=rand(gen, n, V, 2),
                probs=torch.softmax(rand(gen, n, V, V), -1))


# ---------------------------------------------------------------------------- replay: store_batch / bind_store
@pytest.mark.parametrize("masked", [True, False], ids=["mask", "no-mask"])
@pytest.mark.parametrize("form", ["action", "policy_out"])
def test_store_batch_and_bind_store_leave_the_same_ring(form, masked):
    """Same inputs, five stores of 300 rows into a ring of 700 (wraps in the third), terminal flag on the last: all seven
    ring arrays and mem_cntr byte-identical."""
    from ris_vec_marl_amd import VecReplayBuffer
    n, V, cap, steps = 300, 6, 700, 5
    x = store_inputs(n, V, 3)
    act = dict(action=x["action"]) if form == "action" else dict(action=None, policy_out=(x["power"], x["probs"]))
    a, b = VecReplayBuffer(cap, 5, V + 2, V, device=DEV), VecReplayBuffer(cap, 5, V + 2, V, device=DEV)
    launch = b.bind_store(x["state"], act["action"], x["metrics"], x["reward"], x["state_"], x["mask"] if masked else None,
                          policy_out=act.get("policy_out"))
    for t in range(steps):
        for k in ("state", "action", "metrics", "reward", "state_", "power"):
            x[k].mul_(0.9).add_(0.01 * t)                  # bound inputs are re-read on every launch
        a.store_batch(x["state"], act["action"], x["metrics"], x["reward"], x["state_"], t == steps - 1,
                      x["mask"] if masked else None, policy_out=act.get("policy_out"))
        launch(done=t == steps - 1)
    assert a.mem_cntr == b.mem_cntr == steps * n > cap
    assert ring_bytes(a) == ring_bytes(b)
    assert bool(a.terminal_memory.any()) and bool((a.mask_memory != 1).any()) == masked


def test_bind_store_refuses_and_store_batch_converts():
    from ris_vec_marl_amd import VecReplayBuffer
    n, V = 64, 4
    x = store_inputs(n, V, 5)
    clean = [x["state"], x["action"], x["metrics"], x["reward"], x["state_"], x["mask"]]
    ref = VecReplayBuffer(200, 5, V + 2, V, device=DEV)
    ref.store_batch(*clean[:5], False, clean[5])
    ref.store_batch(clean[0], None, *clean[2:5], True, clean[5], policy_out=(x["power"], x["probs"]))
    for kind in KINDS:
        buf = VecReplayBuffer(200, 5, V + 2, V, device=DEV)
        for i in range(len(clean)):                        # one bad argument at a time
            bad = list(clean)
            bad[i] = variant(clean[i], kind)
            with pytest.raises(ValueError):
                buf.bind_store(*bad)
        for i in range(2):
            po = [x["power"], x["probs"]]
            po[i] = variant(po[i], kind)
            with pytest.raises(ValueError):
                buf.bind_store(clean[0], None, *clean[2:], policy_out=tuple(po))
        assert buf.mem_cntr == 0
        # the unbound method takes all of them at once and stores the same rows
        v = [variant(t, kind) for t in clean]
        buf.store_batch(*v[:5], False, v[5])
        buf.store_batch(v[0], None, *v[2:5], True, v[5], policy_out=(variant(x["power"], kind), variant(x["probs"], kind)))
        assert ring_bytes(buf) == ring_bytes(ref), kind
    # per-row done and a bool mask: the unbound-only conveniences
    done = torch.arange(n, device=DEV) % 3 == 0
    a, b = VecReplayBuffer(200, 5, V + 2, V, device=DEV), VecReplayBuffer(200, 5, V + 2, V, device=DEV)
    a.store_batch(*clean[:5], done, clean[5].bool())
    b.store_batch(*clean[:5], done.to(torch.uint8).cpu().numpy(), clean[5])
    assert ring_bytes(a) == ring_bytes(b) and torch.equal(a.terminal_memory[:n], done)


def test_store_twins_agree_where_they_used_to_differ():
    """Slips the shared builder closed, the stricter answer for both twins."""
    from ris_vec_marl_amd import VecReplayBuffer
    n, V = 32, 4
    x = store_inputs(n, V, 7)
    buf = VecReplayBuffer(100, 5, V + 2, V, device=DEV)
    odd = VecReplayBuffer(100, 5, V + 3, V, device=DEV)    # n_actions != n_agents + 2: no policy-output form
    args = (x["state"], None, x["metrics"], x["reward"], x["state_"])
    with pytest.raises(ValueError):                         # only bind_store checked this
        odd.store_batch(*args, policy_out=(x["power"], x["probs"]))
    with pytest.raises(ValueError):
        odd.bind_store(*args, policy_out=(x["power"], x["probs"]))
    args = (x["state"], x["action"], x["metrics"], x["reward"], x["state_"])
    for short in (x["mask"][: n // 2], x["mask"][:, :, :2]):
        with pytest.raises(ValueError):                     # store_batch never checked the mask's rows
            buf.store_batch(*args, False, short)
        with pytest.raises(ValueError):
            buf.bind_store(*args, short)
    with pytest.raises(ValueError):                         # store_batch reshaped: the error was torch's RuntimeError
        buf.store_batch(x["state"][:, :, :4], *args[1:])
    with pytest.raises(ValueError):                         # a strided [n] view: bind_store read it with stride 1
        buf.bind_store(x["state"], x["action"], x["metrics"][:, 0], x["reward"], x["state_"])
    with pytest.raises(ValueError):
        buf.bind_store(x["state"], x["action"], x["metrics"][: n // 2], x["reward"], x["state_"])
    assert buf.mem_cntr == odd.mem_cntr == 0
    # the unbound method reads the same strided view correctly
    buf.store_batch(x["state"], x["action"], x["metrics"][:, 0], x["reward"], x["state_"])
    assert torch.equal(buf.reward_global_memory[:n], x["metrics"][:, 0])


# ---------------------------------------------------------------------------- NOMA: group / bind_group
def _noma_env(E, V, seed):
    from ris_vec_marl_amd import NomaGrouper
    env = make_vec(E, V, 36, seed=seed, yaml=True)
    env.make_new_game(); env.renew_positions(); env.compute_parms(); env.Random_phase(); env.update_channel_gains()
    g = NomaGrouper(env)
    g.config.freeze_recalc_every = 4                        # re-solve at steps 4 and 8, frozen in between
    g.config.min_pair_target = 2
    return env, g


def grouper_bytes(g):
    keys = ("partner", "n_groups", "flags")
    return [g._t[k].cpu().numpy().tobytes() for k in keys] + [g.pair_affinity_hist.cpu().numpy().tobytes(),
                                                              g.unpaired_streak.cpu().numpy().tobytes(), g._calls]


@pytest.mark.parametrize("form", ["p_off01", "power_raw"])
def test_group_and_bind_group_leave_the_same_state(form):
    """One episode of ten steps with re-solves and frozen steps, the env stepped in between so that its global reward
    feeds the next call: partner, n_groups, pair_affinity_hist, unpaired_streak and flags byte-identical."""
    E, V, steps = 500, 8, 10
    gen = torch.Generator(device=DEV); gen.manual_seed(4)
    power = [rand(gen, E, V, 2) * 1.1 for _ in range(steps)]
    states = []
    for bound in (False, True):
        env, g = _noma_env(E, V, 6)
        pw = torch.empty(E, V, 2, device=DEV)
        p01 = torch.empty(E, V, device=DEV)
        kw = dict(power_raw=pw) if form == "power_raw" else dict(p_off01=p01)
        g.begin_episode(3)
        g.refresh_mask()
        launch = g.bind_group(**kw) if bound else (lambda t: g.group(kw.get("p_off01"), t, power_raw=kw.get("power_raw")))
        per_step, solved = [], []
        for t in range(steps):
            pw.copy_(power[t])
            p01.copy_((pw[..., 0].clamp(-0.999, 0.999) + 1) / 2)
            launch(t)
            env.step(pw, g._t["partner"], g._t["n_groups"], None, fused=False, policy_action=True)
            per_step.append(g._t["partner"].cpu().numpy().tobytes())
            solved.append(int(g.info[:, 0].sum()))          # envs that re-solved (`info` is written by group() only)
        if not bound:
            assert solved[0] == E and 0 < sum(solved[1:]) < E * (steps - 1), solved     # re-solves AND frozen steps
        states.append(per_step + grouper_bytes(g))
    assert states[0] == states[1]


def test_bind_group_refuses_and_group_converts():
    E, V = 300, 8
    gen = torch.Generator(device=DEV); gen.manual_seed(9)
    p01, pw, u = rand(gen, E, V).abs(), rand(gen, E, V, 2), rand(gen, E).abs()
    env, g = _noma_env(E, V, 2)
    gain = env.tensors["gain"].clone()
    db = 10 * torch.log10(gain.double().clamp_min(1e-15))
    g.begin_episode(0); g.refresh_mask()
    for kind in KINDS:
        with pytest.raises(ValueError):
            g.bind_group(variant(p01, kind))
        with pytest.raises(ValueError):
            g.bind_group(power_raw=variant(pw, kind))
    with pytest.raises(ValueError):
        g.bind_group(p01, power_raw=pw)                     # one or the other, for both twins
    with pytest.raises(ValueError):
        g.group(p01, 0, power_raw=pw)
    g.config.mask_enable = False
    with pytest.raises(ValueError):
        g.bind_group(p01)                                   # no cached tau / K to bind
    g.config.mask_enable = True
    assert g._calls == 0

    def run(conv, **kw):
        _, h = _noma_env(E, V, 2)
        h.begin_episode(0); h.refresh_mask(gain=conv(gain), gdb15=conv(db, False))
        h.group(conv(p01), 0, gain=conv(gain), gdb12=conv(db, False), gdb15=conv(db, False), u_unstick=conv(u), **kw)
        h.group(None, 1, power_raw=conv(pw), gain=conv(gain))
        return grouper_bytes(h)
    ref = run(lambda x, f32=True: x)
    for kind in KINDS:                                      # float64 dB gains have no wider type to arrive in
        assert run(lambda x, f32=True: x if (kind == "wrong dtype" and not f32) else variant(x, kind)) == ref, kind
    # slips: neither twin checked the rows of these (the kernel reads n_envs of them)
    _, h = _noma_env(E, V, 2)
    h.begin_episode(0); h.refresh_mask()
    for kw in (dict(u_unstick=u[: E // 2]), dict(prev_global=u[: E // 2]), dict(prev_global=u.double()),
               dict(gdb12=db[:, :4]), dict(gain=gain[: E // 2])):
        with pytest.raises(ValueError):
            h.group(p01, 0, **kw)
    assert h._calls == 0 and not h._have_reward
    # a strided [E] view of the metrics is read with its stride
    m = torch.zeros(E, 16, device=DEV); m[:, 0] = -u
    a, b = _noma_env(E, V, 2)[1], _noma_env(E, V, 2)[1]
    for h, prev in ((a, m[:, 0]), (b, (-u).contiguous())):
        h.begin_episode(0); h.refresh_mask(); h.group(p01, 0); h.group(p01, 1, prev_global=prev)
    assert grouper_bytes(a) == grouper_bytes(b) and torch.equal(a._t["last_global"], b._t["last_global"])


def test_group_without_a_mask_is_the_same_through_both_doors():
    """No mask held (begin_episode without refresh_mask): `group()` recomputes tau from the pairing quantile in an extra
    launch on every call; the bound launcher now does the same instead of stopping with an error."""
    E, V = 200, 8
    gen = torch.Generator(device=DEV); gen.manual_seed(1)
    p01 = rand(gen, E, V).abs()
    out = []
    for bound in (False, True):
        _, g = _noma_env(E, V, 8)
        g.begin_episode(0)
        run = g.bind_group(p01) if bound else (lambda t: g.group(p01, t))
        for t in range(3):
            run(t)
        out.append(grouper_bytes(g) + [g.tau.cpu().numpy().tobytes()])
    assert out[0] == out[1]


# ---------------------------------------------------------------------------- the other bound launchers
def test_every_other_bound_launcher_refuses_what_it_cannot_read_in_place():
    from ris_vec_marl_amd import BatchedPolicy, EpisodeMeter, VecReplayBuffer, marshal_actions
    E, V, M, T = 64, 8, 36, 3
    env = make_vec(E, V, M, seed=3, yaml=True)
    env.make_new_game(); env.compute_parms(); env.Random_phase(); env.update_channel_gains()
    gen = torch.Generator(device=DEV); gen.manual_seed(2)
    act, acts, pw, phase = rand(gen, E, 2, V).abs(), rand(gen, T, E, 2, V).abs(), rand(gen, E, V, 2), rand(gen, E, M)
    probs = torch.softmax(rand(gen, E, V, V), -1)
    pt = torch.full((E, V), -1, dtype=torch.int32, device=DEV)
    ng = torch.full((E,), V, dtype=torch.int32, device=DEV)
    replay = VecReplayBuffer(4 * E, 5, V + 2, V, device=DEV)
    meter, policy = EpisodeMeter(env), BatchedPolicy(V, 5, 64, 32, device=DEV)
    t = env.tensors
    outs = (torch.zeros(E, 2, V, device=DEV), torch.zeros(E, V, device=DEV), torch.zeros(E, V * (V + 2), device=DEV))
    for kind in KINDS:
        bad = lambda x: variant(x, kind)                    # noqa: E731
        calls = [lambda: env.bind_step(bad(act), pt, ng), lambda: env.bind_step(act, bad(pt), ng),
                 lambda: env.bind_step(act, pt, bad(ng)),
                 lambda: env.bind_step_many(bad(acts), pt, ng), lambda: env.bind_sarl_step(bad(act), phase),
                 lambda: env.bind_sarl_step(act, bad(phase)), lambda: env.bind_step_store(replay, bad(pw), pt, ng, probs),
                 lambda: env.bind_step_store(replay, pw, pt, ng, bad(probs)),
                 lambda: meter.bind(metrics=bad(t["metrics"]), reward=t["reward"], power_w=t["power_w"]),
                 lambda: meter.bind(metrics=t["metrics"], reward=bad(t["reward"])),
                 lambda: meter.bind(metrics=t["metrics"], reward=t["reward"], power_w=bad(t["power_w"]))]
        for i in range(3):
            o = list(outs)
            o[i] = bad(o[i])
            calls.append(lambda o=o: policy.choose_action(env.observe(), cpu_share_floor=0.1, out=tuple(o)))
            calls.append(lambda o=o: marshal_actions(pw, probs, 0.1, out=tuple(o)))
        for i, call in enumerate(calls):
            with pytest.raises(ValueError):
                call()
                pytest.fail("%s input accepted by bound launcher %d" % (kind, i))
    assert env._steps == 0 and replay.mem_cntr == 0 and meter.n_steps == 0
    # choose_action itself is unbound: obs and mask in any of the three forms give the same draw
    mask = (rand(gen, E, V, V) < 0.5).to(torch.uint8)
    ref = policy.choose_action(env.observe(), mask, cpu_share_floor=0.1)
    for kind in KINDS:
        policy._calls -= 1                                  # the same Philox counter again
        got = policy.choose_action(variant(env.observe(), kind), variant(mask, kind), cpu_share_floor=0.1)
        assert all(torch.equal(x, y) for x, y in zip(got, ref)), kind
