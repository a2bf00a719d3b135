"""GPU sweep of the policy forward -- `BatchedPolicy.forward_heads`: `k_policy_layer1_v4<NT,8,SPLIT16>`, `k_policy_layer1<FPL>`,
`k_policy_heads_v4<NT>`, `k_policy_heads<FPL>` (csrc/k_policy.hip) and `k_policy_mlp<MT>` (csrc/k_policy_mlp.hip) -- over
every template instantiation and every edge of the run-time parameters (tests/policy_forward_shapes.py names the kernels
a case reaches and the edge it is there for; tests/test_policy_forward_host.py proves the table on the host, since the
policy launchers do not report their kernel).  test_policy_hip.py stays at the fixtures and the driver's sizes, against
a float32 forward on the same device.

Per case, against the float64 restatement of the reference's network (tests/policy_forward_ref.py), per agent, with the
project's bars imported and not restated (err < BAR = 2e-5; err <= fused_bar(library err) = max(8 x library, 1e-7), the
library being the same computation by torch on the device, on the same inputs):
  (a) the whole forward in every mode the shape admits, 289 rows: row 0 all zero, row 1 all 1.2;
  (b) layer 1 alone through the C ABI (`risvec_policy_layer1`); where the shape has a split-fp16 form, its three
      float16 K-blocks are exactly what include/risvec.h says of the float32 row;
  (c) the heads alone through the C ABI (`risvec_policy_heads`) on a random `g` drawn on the host: no GEMM library in
      the comparison;
  (d) the outputs of (b), (c) and of `risvec_policy_mlp` lie between 64 sentinel words in front and 64 behind, which
      stay untouched;
  (e) rows are independent, bit for bit, where the arithmetic is the project's own -- (b), (c) and the fused forward:
      row 0 alone and rows 0..32 alone get the bits the 289-row call wrote for them (not asserted for the fp32 / fp16x3
      forwards: rocBLAS may pick another kernel at another row count);
  (f) the refusals: heads LDS one agent past 64 KiB, layer-1 LDS one input past it, 25 heads in the fused form.
Every figure is printed before it is asserted (pytest -s shows them; a green run is in
profiles/policy_forward_margins.txt).  The whole file takes a few seconds."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests import policy_forward_ref as R  # noqa: E402
from tests import policy_forward_shapes as PS  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
SENTINEL = -7.0
F = torch.nn.functional


def T(x):
    return torch.tensor(np.asarray(x)).to(DEV)              # a copy: the shared inputs are read-only arrays


def bits(t):
    """a tensor as integer bit patterns (numpy): equality that tells -0 from 0 and compares NaN"""
    a = t.detach().cpu().contiguous()
    return a.view(torch.int16 if a.dtype == torch.float16 else torch.int32).numpy()


def make(case, weights, gemm=None):
    from ris_vec_marl_amd import BatchedPolicy
    IN, F1, F2, V = case.dims
    pol = BatchedPolicy(V, IN, F1, F2, device=DEV, seed=1, gemm=gemm)
    for a in range(V):
        pol.load_agent_state_dict(a, weights[a])
    return pol


class Guarded:
    """An output of `shape` between PS.GUARD sentinel words (float32) in front and behind, NaN where the kernel must write"""

    def __init__(self, shape, dtype=torch.float32):
        per_word = 4 // torch.empty((), dtype=dtype).element_size()
        self.pad, numel = PS.GUARD * per_word, int(np.prod(shape))
        self.flat = torch.full((numel + 2 * self.pad,), SENTINEL, dtype=dtype, device=DEV)
        self.out = self.flat[self.pad:self.pad + numel].view(*shape)
        self.out.fill_(NAN)
        assert self.out.data_ptr() == self.flat.data_ptr() + 4 * PS.GUARD and self.out.data_ptr() % 16 == 0

    def kept(self):
        return bool((self.flat[:self.pad] == SENTINEL).all()) and bool((self.flat[-self.pad:] == SENTINEL).all()) \
            and bool(torch.isfinite(self.out).all())


def call_layer1(pol, x, split=False):
    """`risvec_policy_layer1` (or its split-fp16 form) on x [n, V, IN] into a guarded buffer"""
    from ris_vec_marl_amd import _native as N
    n, V, F1 = int(x.shape[0]), pol.n_agents, pol.fc1_dims
    buf = Guarded((V, n, 3 * F1), torch.float16) if split else Guarded((V, n, F1))
    fn = N.load().risvec_policy_layer1_split16 if split else N.load().risvec_policy_layer1
    N.check(fn(n, V, pol.input_dims, F1, x.data_ptr(), pol.W1.data_ptr(), pol.b1.data_ptr(), pol.ln1_w.data_ptr(),
               pol.ln1_b.data_ptr(), buf.out.data_ptr(), N.stream(pol.device)))
    return buf


def call_heads(pol, g):
    """`risvec_policy_heads` on g [V, n, fc2] into a guarded buffer"""
    from ris_vec_marl_amd import _native as N
    V, n, H = pol.n_agents, int(g.shape[1]), 4 + pol.n_agents
    buf = Guarded((V, n, H))
    N.check(N.load().risvec_policy_heads(n, V, pol.fc2_dims, H, g.data_ptr(), pol.b2.data_ptr(), pol.ln2_w.data_ptr(),
                                         pol.ln2_b.data_ptr(), pol.Wh.data_ptr(), pol.bh.data_ptr(), buf.out.data_ptr(),
                                         N.stream(pol.device)))
    return buf


def call_mlp(pol, x):
    """`risvec_policy_mlp` with the prepared weights of `pol` into a guarded buffer"""
    from ris_vec_marl_amd import _native as N
    n, V, H = int(x.shape[0]), pol.n_agents, 4 + pol.n_agents
    gram, w1f, frag, unscale, hfrag, hunscale = pol._fused_weights()
    buf = Guarded((V, n, H))
    N.check(N.load().risvec_policy_mlp(n, V, pol.input_dims, pol.fc1_dims, pol.fc2_dims, H, x.data_ptr(), gram.data_ptr(),
                                       w1f.data_ptr(), frag.data_ptr(), unscale.data_ptr(), pol.b2.data_ptr(),
                                       pol.ln2_w.data_ptr(), pol.ln2_b.data_ptr(), hfrag.data_ptr(), hunscale.data_ptr(),
                                       pol.bh.data_ptr(), buf.out.data_ptr(), N.stream(pol.device)))
    return buf


def layer1_torch(pol, x):
    h = torch.baddbmm(pol.b1, x.transpose(0, 1), pol.W1)
    return torch.relu(F.layer_norm(h, (pol.fc1_dims,)) * pol.ln1_w + pol.ln1_b)


def heads_torch(pol, g):
    h = torch.relu(F.layer_norm(g + pol.b2, (pol.fc2_dims,)) * pol.ln2_w + pol.ln2_b)
    return torch.baddbmm(pol.bh, h, pol.Wh)


def check_bars(what, got, lib, refs):
    """got, lib [V, n, K] device tensors against refs (V float64 arrays [n, K]): both bars, per agent"""
    got, lib = got.cpu().numpy(), lib.cpu().numpy()
    assert np.isfinite(got).all(), what
    e = [R.err(got[a], refs[a]) for a in range(len(refs))]
    e_lib = [R.err(lib[a], refs[a]) for a in range(len(refs))]
    r_bar = [x / R.BAR for x in e]
    r_fused = [x / R.fused_bar(y) for x, y in zip(e, e_lib)]
    a = int(np.argmax(r_fused))
    print("policy_forward %-24s err %.3g  library %.3g  err/BAR %.3f  err/fused_bar %.3f (agent %d of %d: err %.3g, library %.3g)"
          % (what, max(e), max(e_lib), max(r_bar), max(r_fused), a, len(refs), e[a], e_lib[a]))
    assert max(e_lib) < R.BAR, what
    assert max(r_bar) < 1.0, what
    assert max(r_fused) <= 1.0, what
    return got


@pytest.mark.parametrize("run", PS.RUNS, ids=[PS.run_id(r) for r in PS.RUNS])
def test_policy_forward(run):
    from ris_vec_marl_amd import BatchedPolicy
    D = R.case_data(*run)
    case = D.case
    IN, F1, F2, V = case.dims
    H, n = 4 + V, PS.ROWS
    tag = "%s %s" % (run[0], PS.case_id(case))
    x, g = T(D.obs), T(D.g)
    assert tuple(x.shape) == (n, V, IN) and not x[0].any() and bool((x[1] == 1.2).all())
    assert all(np.abs(ref).max() > 0.05 for ref in D.heads_64)          # widened heads on live features: not a zero output

    # ---- (a) the whole forward, every admissible mode
    assert BatchedPolicy(V, IN, F1, F2, device=DEV).gemm == case.modes[0]
    for mode in BatchedPolicy.GEMM_MODES:
        if mode not in case.modes:
            with pytest.raises(ValueError):
                BatchedPolicy(V, IN, F1, F2, device=DEV, gemm=mode)
    pols = {}
    for mode in case.modes:
        pol = pols[mode] = make(case, D.weights, mode)
        assert pol.gemm == mode
        heads = pol.forward_heads(x)
        assert tuple(heads.shape) == (V, n, H)
        check_bars("%s %s" % (tag, mode), heads, pol.forward_heads_torch(x), D.heads_64)
    pol = pols["fp32"]

    # ---- (b) layer 1 alone, (d) its guards, (e) its rows
    b1 = call_layer1(pol, x)
    assert b1.kept(), tag
    check_bars("%s layer1" % tag, b1.out, layer1_torch(pol, x), D.h1_64)
    for k in PS.SHORT_ROWS:
        short = call_layer1(pol, x[:k].contiguous())
        assert short.kept() and np.array_equal(bits(short.out), bits(b1.out[:, :k])), (tag, k)
    if "fp16x3" in case.modes:
        s16 = call_layer1(pol, x, split=True)
        assert s16.kept(), tag
        h32 = b1.out
        hi = h32.to(torch.float16)
        assert torch.equal(s16.out[..., :F1], hi), tag
        assert torch.equal(s16.out[..., F1:2 * F1], (hi.float() * 0.03125).to(torch.float16)), tag
        assert torch.equal(s16.out[..., 2 * F1:], ((h32 - hi.float()) * 64.0).to(torch.float16)), tag
        for k in PS.SHORT_ROWS:
            short = call_layer1(pol, x[:k].contiguous(), split=True)
            assert short.kept() and np.array_equal(bits(short.out), bits(s16.out[:, :k])), (tag, k)

    # ---- (c) the heads alone on the host's g, (d), (e)
    hd = call_heads(pol, g)
    assert hd.kept(), tag
    check_bars("%s heads" % tag, hd.out, heads_torch(pol, g), D.heads_g_64)
    for k in PS.SHORT_ROWS:
        short = call_heads(pol, g[:, :k].contiguous())
        assert short.kept() and np.array_equal(bits(short.out), bits(hd.out[:, :k])), (tag, k)

    # ---- the fused launch: (d) through the C ABI, (e) through the class
    if "fused" in case.modes:
        fz = pols["fused"]
        whole = fz.forward_heads(x)
        direct = call_mlp(fz, x)
        assert direct.kept() and np.array_equal(bits(direct.out), bits(whole)), tag
        for k in PS.SHORT_ROWS:
            short = fz.forward_heads(x[:k].contiguous())
            assert tuple(short.shape) == (V, k, H) and np.array_equal(bits(short), bits(whole[:, :k])), (tag, k)
            short = call_mlp(fz, x[:k].contiguous())
            assert short.kept() and np.array_equal(bits(short.out), bits(whole[:, :k])), (tag, k)


def test_refusals():
    """(f): every one an error raised before any launch"""
    from ris_vec_marl_amd import BatchedPolicy
    from ris_vec_marl_amd import _native as N
    lib = N.load()
    IN, F1, F2, V = PS.HEADS_LDS_OVER
    pol = BatchedPolicy(V, IN, F1, F2, device=DEV, gemm="fp32")
    x = torch.zeros(4, V, IN, device=DEV)
    with pytest.raises(ValueError):
        pol.forward_heads(x)
    torch.cuda.synchronize()
    g, out = torch.zeros(V, 4, F2, device=DEV), torch.full((V, 4, 4 + V), SENTINEL, device=DEV)
    args = (g.data_ptr(), pol.b2.data_ptr(), pol.ln2_w.data_ptr(), pol.ln2_b.data_ptr(), pol.Wh.data_ptr(), pol.bh.data_ptr(),
            out.data_ptr(), N.stream(pol.device))
    assert lib.risvec_policy_heads(4, V, F2, 4 + V, *args) == N.ERR_SHAPE
    assert bool((out == SENTINEL).all())
    IN, F1 = PS.LAYER1_LDS_OVER
    p = x.data_ptr()
    assert lib.risvec_policy_layer1(4, 1, IN, F1, p, p, p, p, p, p, None) == N.ERR_SHAPE
    IN, F1, F2, V = PS.FUSED_H_OVER
    with pytest.raises(ValueError):
        BatchedPolicy(V, IN, F1, F2, device=DEV, gemm="fused")
    assert BatchedPolicy(V, IN, F1, F2, device=DEV).gemm == "fp16x3"
    assert lib.risvec_policy_mlp_supported(IN, F1, F2, 4 + V) == 0 and lib.risvec_policy_mlp_supported(IN, F1, F2, 24) == 1
