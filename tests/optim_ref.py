"""float64 restatement of `clip_grad_norm_` -> `torch.optim.Adam` -> the Polyak blend, statement by statement, from float32
inputs, and the running-error bars the float32 forms are held to.  u = 2^-24 (half a unit in the last place of 1).

The clip coefficient is an ARGUMENT of `adam_ref`, so the norm and the element-wise arithmetic are judged separately:

    norm_ref(grads)                  sqrt(sum g^2) in float64.  Bar NORM_K u = 4 u relative: the float32 form rounds every
                                     square once (u on each term, all positive, so u on the sum), adds them in float64 (no
                                     visible error), takes the root in float64 (the u halves) and rounds it to float32 once
                                     (u): 1.5 u at first order, 4 u with the rule "roundings plus two".

    adam_ref(p, grad, m, v, coef, ...) with gc = grad coef, G = |gc| + |weight_decay p| (the terms of g), in float64:
        g  = gc + weight_decay p
        m' = m + (g - m)(1 - beta1)            terms  b1 |m|, (1 - b1) G          -> Tm = beta1 |m| + (1 - beta1) G
        v' = v beta2 + (1 - beta2) g g         terms  b2 v, (1 - b2) G^2          (v' itself: all terms >= 0)
        d  = sqrt(v') / sqrt(1 - beta2^t) + eps
        U  = step_size m' / d                  p' = p - U

    Each bar is K u times the sum of the absolute values of the terms of its statement, K = the statement's float32
    roundings plus two (the two cover the roundings of the inputs it takes from the statements before it and of its
    float32 constants):

        m   3 roundings (g - m, the product, the sum), each at most u on a term that is at most Tm + |m'| <= 2 Tm; the
            input g carries 1 rounding (3 with weight decay) weighted by (1 - beta1), the constant fl32(1 - beta1) one more
            on the product.  Bar: M_K u (|m| + G), M_K = 4: first order the error is below 3 u Tm <= 3 u (|m| + G).
        v   4 roundings (v beta2, (1 - beta2) g, its product with g, the sum) on positive terms, plus the constants'
            two: below 4 u v' at first order.  Bar: V_K u (|v| + G^2), V_K = 4.  G^2 is the sum of the absolute values of
            the terms of g g: without weight decay it is g^2; with it g = gc + weight_decay p may cancel, and g's own
            rounding error, up to 3 u G, enters g g as 6 u |g| G, which no multiple of u g^2 covers (seen on the GPU: 3.8
            times a bar on g^2 at the SARL critic's LayerNorm weights).
        p   the final subtraction rounds once: u |p'|.  The update term U takes m' (3 u Tm / d step_size as above, plus
            the same again for g's own roundings with weight decay), and relative errors of v' 4 u -> sqrt 2 u + 1 u,
            / bc2_sqrt 2 u (the quotient and the constant), + eps 1 u, step_size m 2 u, the quotient 1 u: 9 u |U|.  With
            T = step_size Tm / d >= |U|: 6 u T + 9 u |U| <= 15 u T.  Bar: u |p'| + P_K u T, P_K = 16.

    Every rounding also has gradual underflow's absolute error, at most half the spacing 2^-149 of the subnormals: a
    gradient of 1e-12 times a small coefficient squares to below 2^-126.  The m and v bars therefore carry K 2^-149 more,
    the param bar 2^-149 (an underflow in v moves sqrt(v) by at most 2^-74, nothing beside eps).

    PyTorch's own float32 kernels (CPU; `test_batched_adam_host.py` feeds them the same inputs, rebased on their float32
    state before every step, the coefficient from their own float32 norm) must stay inside the same element-wise bars:
    that shows the bars are not tighter than float32 permits.  Observed there, as the largest |error| / bar over all
    steps and cases: m 0.23, v 0.47, param 0.99 (the final rounding alone can reach u |p'|); their norm (float32 accumulation) was within
    2.3 u here, ours is held to 4 u.  The kernel on an MI355X: m 0.24, v 0.53, param 0.99, norm 0.97 u.
"""
import torch

U32 = 2.0 ** -24
NORM_K, M_K, V_K, P_K = 4, 4, 4, 16
TINY = 2.0 ** -149                                            # the spacing of float32's subnormals


def norm_ref(grads) -> float:
    """sqrt(sum of squares) over a list of float32 tensors, in float64."""
    return float(sum((g.detach().double() ** 2).sum() for g in grads).sqrt())


def coef_f32(norm, max_norm):
    """`clip_grad_norm_`'s coefficient from a float32 norm, in float32 as it states it (None: no clipping)."""
    if max_norm is None:
        return 1.0
    n = torch.as_tensor(norm, dtype=torch.float32)
    return float(torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (n + torch.tensor(1e-6, dtype=torch.float32)), max=1.0))


def adam_ref(p, grad, m, v, coef, lr, betas, eps, weight_decay, t):
    """One Adam step (step count t >= 1) of one tensor in float64 from float32 inputs.  -> dict of float64 tensors: the new
    "p", "m", "v", the clipped gradient "gc", and the bars "p_bar", "m_bar", "v_bar"."""
    b1, b2 = betas
    p, grad, m, v = (x.detach().double().cpu() for x in (p, grad, m, v))
    gc = grad * float(coef)
    g = gc + weight_decay * p if weight_decay != 0 else gc
    G = gc.abs() + (weight_decay * p).abs() if weight_decay != 0 else gc.abs()
    m1 = m + (g - m) * (1 - b1)
    v1 = v * b2 + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    step_size = lr / bc1
    d = v1.sqrt() / bc2 ** 0.5 + eps
    upd = step_size * m1 / d
    p1 = p - upd
    T = step_size * (b1 * m.abs() + (1 - b1) * G) / d
    return {"p": p1, "m": m1, "v": v1, "gc": gc,
            "m_bar": M_K * (U32 * (m.abs() + G) + TINY), "v_bar": V_K * (U32 * (v.abs() + G * G) + TINY),
            "p_bar": U32 * p1.abs() + P_K * U32 * T + TINY}


def worst_ratio(got, want, bar) -> float:
    """max |got - want| / bar over the elements (0 / 0 counts as 0; a NaN anywhere gives NaN)."""
    err = (got.detach().double().cpu() - want).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bar)
    return float(r.max()) if not torch.isnan(r).any() else float("nan")
