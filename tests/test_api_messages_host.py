"""The text of `risvec_last_error()` for the argument checks that the learner-side entry points share (the per-net table of
`risvec_marl_critic` / `risvec_local_critics` and their output checks, the stream and workspace sizes and the float
pointers of the three `*_pack` entry points, `risvec_soft_update`, `risvec_adam_step`'s pointers, the state pointers of
`risvec_sarl_step` / `risvec_sarl_rollout`, the n_envs / n_veh range of the marshalling entry points, the lane limit of `risvec_mobility`): the code AND the
message, byte for byte, one fault per call.  The pointers are aligned host addresses that are only checked, never
dereferenced: nothing here touches a device."""
import ctypes as C

import ris_vec_marl_amd as rv
from ris_vec_marl_amd import _native as N
from tests.test_batched_adam_host import _call as adam_call

FAKE = 0x7F0000001000                                         # 16-byte aligned, never dereferenced
MARL = (3, 2, 32, 128, 128)                                   # (state, action, fc1, fc2, fc3): a stream of 82 rows of 1 KiB
LOCAL = (3, 5, 32, 128, 128)                                  # 3 agents: action_dims = n_agents + 2; the same 82 rows
STREAM = 83968
ACTOR = (10, 32, 128, 4)                                      # (in, fc1, fc2, n_actions)
CRITIC = (10, 32, 128, 128, 4)                                # (in, fc1, fc2, fc3, n_actions)
NET_PTRS = ("wstream", "scales", "b1", "b2", "b3", "qw")


def says(rc, code, text):
    msg = N.load().risvec_last_error().decode()
    assert (rc, msg) == (code, text)


def critic_nets(count, bad_net, wb=STREAM, **kw):
    arr = (N.RisVecMarlCriticNet * count)()
    for c in range(count):
        arr[c] = N.RisVecMarlCriticNet(FAKE, STREAM, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE)
    arr[bad_net].wstream_bytes = wb
    for k, v in kw.items():
        setattr(arr[bad_net], k, v)
    return arr


def shared_critic_checks(fn, count, nets_at, call):
    """The per-net loop and the output / epilogue checks, which `risvec_marl_critic` and `risvec_local_critics` word alike."""
    for k in nets_at:
        says(call(bad_net=k, wb=STREAM - 1024), N.ERR_ARG,
             "%s: nets[%d].wstream_bytes=82944, this shape's weight stream has 83968" % (fn, k))
        for f in NET_PTRS:
            says(call(bad_net=k, **{f: None}), N.ERR_ARG, "%s: nets[%d].%s is NULL" % (fn, k, f))
            says(call(bad_net=k, **{f: FAKE + 4}), N.ERR_ARG, "%s: nets[%d].%s is not 16-byte aligned" % (fn, k, f))
        says(call(bad_net=k, qb=None), N.ERR_ARG, "%s: nets[%d].qb is NULL" % (fn, k))
    says(call(q1=None, q2=None, y=None, lp=None, li=None), N.ERR_ARG, "%s: q1, q2 and y are all NULL" % fn)
    says(call(n_nets=1), N.ERR_ARG, "%s: q2 needs n_nets == 2" % fn)
    says(call(rw=None), N.ERR_ARG, "%s: y needs reward and done" % fn)
    says(call(dn=None), N.ERR_ARG, "%s: y needs reward and done" % fn)
    says(call(coef=None), N.ERR_ARG, "%s: logp_power / logp_intent need coef" % fn)
    says(call(coef=None, lp=None), N.ERR_ARG, "%s: logp_power / logp_intent need coef" % fn)
    says(call(y=None), N.ERR_ARG, "%s: logp_power / logp_intent need y" % fn)
    says(call(y=None, li=None), N.ERR_ARG, "%s: logp_power / logp_intent need y" % fn)
    says(call(gamma=float("nan")), N.ERR_ARG, "%s: gamma=nan must be finite" % fn)
    says(call(gamma=float("inf")), N.ERR_ARG, "%s: gamma=inf must be finite" % fn)
    says(call(gamma=float("-inf"), q1=None, q2=None, y=None, lp=None, li=None), N.ERR_ARG, "%s: q1, q2 and y are all NULL" % fn)


def test_marl_critic_messages():
    lib, fn, p = N.load(), "risvec_marl_critic", FAKE

    def call(n_nets=2, bad_net=1, wb=STREAM, st=p, ac=p, rw=p, dn=p, gamma=0.99, coef=p, lp=p, li=p, q1=p, q2=p, y=p, **kw):
        nets = critic_nets(2, bad_net, wb, **kw)
        return lib.risvec_marl_critic(4, *MARL, n_nets, C.cast(nets, C.c_void_p), st, ac, rw, dn, gamma, coef, lp, li, q1, q2, y, None)
    shared_critic_checks(fn, 2, (0, 1), call)
    says(call(st=None), N.ERR_ARG, "%s: state or action is NULL" % fn)
    # the second net of a one-net call is not looked at; the first fault in the argument order decides
    says(call(n_nets=1, q2=None, bad_net=1, b1=None, gamma=float("nan")), N.ERR_ARG, "%s: gamma=nan must be finite" % fn)
    says(call(bad_net=0, wb=0, b1=None), N.ERR_ARG, "%s: nets[0].wstream_bytes=0, this shape's weight stream has 83968" % fn)
    says(call(bad_net=1, qb=None, qw=None), N.ERR_ARG, "%s: nets[1].qw is NULL" % fn)
    says(call(bad_net=1, qb=None, ac=None), N.ERR_ARG, "%s: nets[1].qb is NULL" % fn)


def test_local_critics_messages():
    lib, fn, p, V = N.load(), "risvec_local_critics", FAKE, 3

    def call(n_nets=2, bad_net=1, wb=STREAM, obs=p, ac=p, hd=None, pw=None, rw=p, dn=p, gamma=0.99, coef=p, lp=p, li=p, q1=p, q2=p,
             y=p, **kw):
        nets = critic_nets(2 * V, bad_net, wb, **kw)
        return lib.risvec_local_critics(4, V, *LOCAL, n_nets, C.cast(nets, C.c_void_p), obs, ac, hd, pw, rw, dn, gamma, coef, lp, li,
                                        q1, q2, y, None)
    shared_critic_checks(fn, 2 * V, (0, 3, 5), call)          # nets[3]: the second agent's net 2; nets[5]: the last agent's
    says(call(obs=None), N.ERR_ARG, "%s: obs is NULL" % fn)
    # with one net per agent the table has n_agents entries: nets[3] and up are not looked at
    says(call(n_nets=1, q2=None, bad_net=3, b1=None, gamma=float("nan")), N.ERR_ARG, "%s: gamma=nan must be finite" % fn)
    says(call(n_nets=1, q2=None, bad_net=2, b1=None), N.ERR_ARG, "%s: nets[2].b1 is NULL" % fn)
    # the input-form checks stand between the table and the output checks
    says(call(bad_net=4, qb=None, ac=None), N.ERR_ARG, "%s: nets[4].qb is NULL" % fn)
    says(call(ac=None, q1=None, q2=None, y=None, lp=None, li=None), N.ERR_ARG, "%s: action and heads are both NULL" % fn)


def test_sarl_actor_pack_messages():
    lib, fn, p = N.load(), "risvec_sarl_actor_pack", FAKE
    need = lib.risvec_sarl_actor_pack_workspace(*ACTOR)
    assert need == 416

    def call(wb=73728, kb=need, ws=p, wk=p):
        return lib.risvec_sarl_actor_pack(*ACTOR, p, p, p, p, p, p, ws, wb, p, wk, kb, None)
    says(call(wb=73728 - 1024), N.ERR_ARG, "%s: wstream_bytes=72704, this shape's weight stream has 73728" % fn)
    says(call(kb=need - 1), N.ERR_ARG, "%s: workspace_bytes=415, this shape needs 416 (risvec_sarl_actor_pack_workspace)" % fn)
    says(call(wb=0, kb=0), N.ERR_ARG, "%s: wstream_bytes=0, this shape's weight stream has 73728" % fn)
    says(call(wb=0, wk=None), N.ERR_ARG, "%s: workspace is NULL" % fn)


def test_sarl_critic_pack_messages():
    lib, fn, p = N.load(), "risvec_sarl_critic_pack", FAKE
    need = lib.risvec_sarl_critic_pack_workspace(*CRITIC)
    nbytes = lib.risvec_sarl_critic_stream_bytes(*CRITIC)
    assert (need, nbytes) == (1552, 92160)
    names = ("W1", "b1", "W2", "Wav", "W3", "ws", "sc", "wk")

    def call(wb=nbytes, kb=need, **kw):
        a = {n: kw.get(n, p) for n in names}
        return lib.risvec_sarl_critic_pack(*CRITIC, a["W1"], a["b1"], a["W2"], a["Wav"], a["W3"], a["ws"], wb, a["sc"], a["wk"], kb, None)
    for k, name in (("W1", "W1"), ("b1", "b1"), ("W2", "W2"), ("Wav", "Wav"), ("W3", "W3"), ("sc", "scales")):
        says(call(**{k: None}), N.ERR_ARG, "%s: %s is NULL" % (fn, name))
        says(call(**{k: p + 2}), N.ERR_ARG, "%s: %s is not 4-byte aligned" % (fn, name))
        assert call(**{k: p + 4}, kb=0) == N.ERR_ARG and b"workspace_bytes" in lib.risvec_last_error()      # 4 bytes are enough
    says(call(W3=None, W1=p + 1), N.ERR_ARG, "%s: W1 is not 4-byte aligned" % fn)     # in the order of the arguments
    says(call(ws=None, sc=None), N.ERR_ARG, "%s: scales is NULL" % fn)                # scales before the 16-byte pointers
    says(call(ws=None), N.ERR_ARG, "%s: wstream is NULL" % fn)
    says(call(wk=p + 8), N.ERR_ARG, "%s: workspace is not 16-byte aligned" % fn)
    says(call(wb=nbytes + 1024), N.ERR_ARG, "%s: wstream_bytes=93184, this shape's weight stream has 92160" % fn)
    says(call(kb=need - 16), N.ERR_ARG, "%s: workspace_bytes=1536, this shape needs 1552 (risvec_sarl_critic_pack_workspace)" % fn)
    says(call(wb=1, kb=1), N.ERR_ARG, "%s: wstream_bytes=1, this shape's weight stream has 92160" % fn)


def test_marl_critic_pack_messages():
    lib, fn, p = N.load(), "risvec_marl_critic_pack", FAKE
    need = lib.risvec_marl_critic_pack_workspace(*MARL, 2)
    assert need == 768

    def call(n_nets=2, bad_net=1, wb=STREAM, wk=p, kb=need, **kw):
        arr = (N.RisVecMarlCriticPackNet * 2)()
        for c in range(2):                                    # distinct streams and scales per net
            arr[c] = N.RisVecMarlCriticPackNet(p, p, p, p + 64 + 128 * c, STREAM, p + 32 + 128 * c)
        arr[bad_net].wstream_bytes = wb
        for k, v in kw.items():
            setattr(arr[bad_net], k, v)
        return lib.risvec_marl_critic_pack(*MARL, n_nets, C.cast(arr, C.c_void_p), wk, kb, None)
    for net in (0, 1):
        for f in ("W1", "W2", "W3", "scales"):
            says(call(bad_net=net, **{f: None}), N.ERR_ARG, "%s: nets[%d].%s is NULL" % (fn, net, f))
            says(call(bad_net=net, **{f: p + 2}), N.ERR_ARG, "%s: nets[%d].%s is not 4-byte aligned" % (fn, net, f))
        says(call(bad_net=net, wstream=None), N.ERR_ARG, "%s: nets[%d].wstream is NULL" % (fn, net))
        says(call(bad_net=net, wstream=p + 8), N.ERR_ARG, "%s: nets[%d].wstream is not 16-byte aligned" % (fn, net))
        says(call(bad_net=net, wb=STREAM + 1024), N.ERR_ARG,
             "%s: nets[%d].wstream_bytes=84992, this shape's weight stream has 83968" % (fn, net))
        says(call(bad_net=net, wb=-1), N.ERR_ARG, "%s: nets[%d].wstream_bytes=-1, this shape's weight stream has 83968" % (fn, net))
    says(call(bad_net=1, wstream=None, scales=None), N.ERR_ARG, "%s: nets[1].scales is NULL" % fn)    # floats before the stream
    says(call(bad_net=0, wb=0, wstream=p + 4), N.ERR_ARG, "%s: nets[0].wstream is not 16-byte aligned" % fn)
    says(call(bad_net=1, wb=0, wk=None), N.ERR_ARG, "%s: nets[1].wstream_bytes=0, this shape's weight stream has 83968" % fn)
    says(call(n_nets=1, bad_net=1, W1=None, kb=0), N.ERR_ARG,
         "%s: workspace_bytes=0, this call needs 384 (risvec_marl_critic_pack_workspace)" % fn)
    says(call(wk=None), N.ERR_ARG, "%s: workspace is NULL" % fn)
    says(call(kb=need - 1), N.ERR_ARG, "%s: workspace_bytes=767, this call needs 768 (risvec_marl_critic_pack_workspace)" % fn)
    says(call(wstream=p + 64, kb=0), N.ERR_ARG, "%s: nets[0].wstream and nets[1].wstream are the same buffer" % fn)


def test_soft_update_messages():
    lib, fn, p = N.load(), "risvec_soft_update", FAKE

    def call(n=2, on=(p, p + 64), tg=(p + 128, p + 192), ne=(3, 7)):
        k = len(on)
        return lib.risvec_soft_update(n, (C.c_void_p * k)(*on), (C.c_void_p * k)(*tg), (C.c_int64 * k)(*ne), 0.005, 0.995, None)
    # 32 is the launch limit that `_weights.soft_update_tensors` splits at
    says(call(n=33, on=(p,) * 33, tg=(p + 128,) * 33, ne=(1,) * 33), N.ERR_SHAPE, "%s: n_tensors=33 outside [1, 32]" % fn)
    says(call(n=0), N.ERR_SHAPE, "%s: n_tensors=0 outside [1, 32]" % fn)
    says(call(on=(p, None)), N.ERR_ARG, "%s: online[1] or target[1] is NULL" % fn)
    says(call(tg=(None, p + 192)), N.ERR_ARG, "%s: online[0] or target[0] is NULL" % fn)
    says(call(on=(p + 2, p + 64)), N.ERR_ARG, "%s: online[0] or target[0] is not 4-byte aligned" % fn)
    says(call(tg=(p + 128, p + 193)), N.ERR_ARG, "%s: online[1] or target[1] is not 4-byte aligned" % fn)
    says(call(tg=(p + 128, p + 64)), N.ERR_ARG, "%s: online[1] and target[1] are the same tensor" % fn)
    says(call(ne=(3, 0), on=(p, None)), N.ERR_SHAPE, "%s: numel[1]=0 outside [1, 2^40]" % fn)


def test_adam_step_pointer_messages():
    lib, fn = N.load(), "risvec_adam_step"
    buf = (C.c_char * (1 << 17))()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16

    def edit(i, name, value):
        return lambda t: setattr(t[i], name, value(getattr(t[i], name)) if callable(value) else value)
    for name in ("param", "grad", "exp_avg", "exp_avg_sq"):
        says(adam_call(lib, p, tens=edit(1, name, None)), N.ERR_ARG, "%s: tensors[1].%s is NULL" % (fn, name))
        says(adam_call(lib, p, tens=edit(2, name, lambda a: a + 2)), N.ERR_ARG, "%s: tensors[2].%s is not 4-byte aligned" % (fn, name))
    says(adam_call(lib, p, tens=edit(0, "target", lambda a: a + 1)), N.ERR_ARG, "%s: tensors[0].target is not 4-byte aligned" % fn)
    # a NULL target is no fault: the call gets as far as the last check
    says(adam_call(lib, p, tens=edit(0, "target", None), partials_bytes=8), N.ERR_ARG,
         "%s: partials_bytes=8, this call needs 32 (risvec_adam_workspace)" % fn)
    says(adam_call(lib, p, tens=lambda t: setattr(t[0], "exp_avg_sq", t[0].exp_avg)), N.ERR_ARG,
         "%s: tensors[0].exp_avg and .exp_avg_sq are the same tensor" % fn)
    # a misaligned pointer is named before the pointer after it that repeats an earlier one
    says(adam_call(lib, p, tens=lambda t: (setattr(t[0], "grad", t[0].grad + 2), setattr(t[0], "exp_avg", t[0].param))), N.ERR_ARG,
         "%s: tensors[0].grad is not 4-byte aligned" % fn)
    says(adam_call(lib, p, null=("norms",)), N.ERR_ARG, "%s: norms is NULL" % fn)
    says(adam_call(lib, p, off={"norms": 2}), N.ERR_ARG, "%s: norms is not 4-byte aligned" % fn)


STATE_PTRS = ("h_r", "theta", "b", "pl", "gain", "data_buf", "rate", "data_t", "data_p", "reward", "over_power", "over_data",
              "metrics")


def sarl_state(skip=None, misalign=None, obs=True):
    s = N.RisVecState()
    s.abi_version, s.struct_bytes = N.ABI_VERSION, C.sizeof(N.RisVecState)
    s.n_envs, s.n_veh, s.n_ris, s.control_bit = 4, 8, 40, 3
    for k in STATE_PTRS + (("obs",) if obs else ()):
        if k != skip:
            setattr(s, k, FAKE + (8 if k == misalign else 0))
    return s


def test_sarl_step_and_rollout_state_messages():
    lib = N.load()
    prm = rv.SarlParams().to_c()
    r = N.RisVecSarlRollout()
    r.struct_bytes = C.sizeof(N.RisVecSarlRollout)
    r.mu, r.action, r.phase, r.obs_full = FAKE, FAKE, FAKE, FAKE

    def step(s, flags=N.STEP_OBS, ap=FAKE):
        return lib.risvec_sarl_step(C.byref(s), C.byref(prm), ap, None, None, 0, 0, flags, None)

    def rollout(s, flags=0):
        return lib.risvec_sarl_rollout(C.byref(s), C.byref(prm), C.byref(r), None, 0, 0, flags, None)
    for fn, call in (("risvec_sarl_step", step), ("risvec_sarl_rollout", rollout)):
        for k in STATE_PTRS + ("obs",):
            says(call(sarl_state(skip=k)), N.ERR_ARG, "%s: state.%s is NULL" % (fn, k))
            says(call(sarl_state(misalign=k)), N.ERR_ARG, "%s: state.%s is not 16-byte aligned" % (fn, k))
        says(call(sarl_state(), flags=N.STEP_METRICS), N.ERR_ARG, "%s: unknown flag bits 0x%x" % (fn, N.STEP_METRICS))
        says(call(sarl_state(skip="pl", misalign="b")), N.ERR_ARG, "%s: state.b is not 16-byte aligned" % fn)
    # the action is looked at before the state; without RISVEC_STEP_OBS the step asks for no obs
    says(step(sarl_state(skip="h_r"), ap=None), N.ERR_ARG, "risvec_sarl_step: action_power is NULL")
    # the step names a missing pointer before the unknown flag, the rollout the flag first
    says(step(sarl_state(skip="gain"), flags=N.STEP_OBS | N.STEP_METRICS), N.ERR_ARG, "risvec_sarl_step: state.gain is NULL")
    says(step(sarl_state(obs=False), flags=N.STEP_METRICS), N.ERR_ARG,
         "risvec_sarl_step: unknown flag bits 0x%x" % N.STEP_METRICS)
    says(rollout(sarl_state(skip="gain"), flags=N.STEP_METRICS), N.ERR_ARG,
         "risvec_sarl_rollout: unknown flag bits 0x%x" % N.STEP_METRICS)
    r.mu = 0
    says(rollout(sarl_state(skip="gain")), N.ERR_ARG, "risvec_sarl_rollout: rollout.mu is NULL")


def test_marshalling_dims_messages():
    lib, p = N.load(), FAKE
    calls = {
        "risvec_marshal_actions": lambda E, V, pr=p: lib.risvec_marshal_actions(E, V, pr, None, 0.0, None, None, None, None),
        "risvec_policy_sample": lambda E, V, pr=p: lib.risvec_policy_sample(E, V, 0, p, None, p, None, None, None, 0, 0, 0.0, pr, p,
                                                                            None, None, None, None, None),
        "risvec_episode_clear": lambda E, V, pr=p: lib.risvec_episode_clear(E, V, pr, None),
    }
    for fn, call in calls.items():
        says(call(0, 8), N.ERR_SHAPE, "%s: n_envs=0 must be >= 1" % fn)
        says(call(-2, 0), N.ERR_SHAPE, "%s: n_envs=-2 must be >= 1" % fn)
        says(call(4, 0), N.ERR_SHAPE, "%s: n_veh=0 outside [1,64]" % fn)
        says(call(4, 65), N.ERR_SHAPE, "%s: n_veh=65 outside [1,64]" % fn)
        says(call(4, 65, None), N.ERR_SHAPE, "%s: n_veh=65 outside [1,64]" % fn)
    says(calls["risvec_marshal_actions"](4, 8, None), N.ERR_ARG, "risvec_marshal_actions: power_raw is NULL")
    says(calls["risvec_policy_sample"](4, 8, p + 4), N.ERR_ARG, "risvec_policy_sample: power_raw is not 16-byte aligned")
    says(calls["risvec_episode_clear"](4, 8, None), N.ERR_ARG, "risvec_episode_clear: acc is NULL")
    says(calls["risvec_episode_clear"](1 << 27, 64), N.ERR_SHAPE, "risvec_episode_clear: n_envs*(17+n_veh) must stay below 2^31")


def test_mobility_refuses_more_than_four_lanes():
    """A move may draw 2 * n_lanes numbers and a u_turn row (and the two Philox sites) hold 8: with more than four lanes per
    direction `risvec_mobility` refuses, as `risvec_reset` does, before anything is launched.  1...4 lanes pass the check
    (the next fault, a missing state pointer, is named instead)."""
    lib, fn = N.load(), "risvec_mobility"
    s = N.RisVecState()
    s.abi_version, s.struct_bytes = N.ABI_VERSION, C.sizeof(N.RisVecState)
    s.n_envs, s.n_veh, s.n_ris, s.control_bit = 4, 8, 40, 3
    s.pos, s.dir, s.vel = FAKE, FAKE, FAKE

    def call(n, u=FAKE, nu=FAKE):
        lanes = {k: [100.0 + i for i in range(n)] for k in ("up_lanes", "down_lanes", "left_lanes", "right_lanes")}
        return lib.risvec_mobility(C.byref(s), C.byref(rv.EnvParams().to_c(lanes, 400, 400)), u, nu, 0, 1, None)
    for n in (5, 6, 7, 8):
        for u in (FAKE, None):                                # injected and Philox draws alike
            says(call(n, u=u), N.ERR_UNSUPPORTED,
                 "%s: n_lanes=%d: a move may need 2*n_lanes turn draws and u_turn rows hold 8 (at most 4 lanes per direction)" % (fn, n))
    s.vel = None
    for n in (1, 2, 3, 4):
        says(call(n), N.ERR_ARG, "%s: state.vel is NULL" % fn)
    says(call(5), N.ERR_ARG, "%s: state.vel is NULL" % fn)    # in the order of the checks: the state's pointers first
