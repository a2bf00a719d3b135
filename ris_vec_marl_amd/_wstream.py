"""How the weight streams of the hand-written MLP kernels are laid out, as far as they share it on the host: the scaled
float16 hi + lo split and the MFMA fragment orders of the critics' streams.  The device side of the same scheme is
described in csrc/risvec_mfma.hpp and csrc/risvec_pack.hpp.  Who owns the weights a stream is built from, and the Polyak
blend of a target network, are `_weights`' subject; its blend functions stay importable from here.
"""
from __future__ import annotations

import torch

from ._weights import polyak_pairs, polyak_tau, soft_update_tensors  # noqa: F401

_WAVES = 4                        # wavefronts of a workgroup: each owns a quarter of every layer's output features


def centre_fc1(W1: torch.Tensor, b1: torch.Tensor) -> torch.Tensor:
    """[input_dims + 1, fc1] float64: the fc1 weight (as [in, out]) with the bias as one more input row, every row
    centred over the feature axis -- the pre-activation it produces has mean 0 over the features for any input."""
    wb = torch.cat([W1.double().T, b1.double()[None, :]], 0)
    return wb - wb.mean(-1, keepdim=True)


def _split_scaled(w: torch.Tensor, target: float = 64.0):
    """(hi, lo, 2^-s): w 2^s with its largest entry in [target, 2 target), split into float16 hi + lo (the scaling keeps lo
    in the float16 normal range; powers of two cancel exactly)."""
    amax = w.abs().amax().clamp_min(1e-30)
    shift = torch.floor(torch.log2(target / amax)).clamp(-40, 40)
    ws = (w.double() * torch.exp2(shift)).float()
    hi = ws.to(torch.float16)
    return hi, (ws - hi.float()).to(torch.float16), torch.exp2(-shift).float()


# A fragments [tiles, k-steps, 2 (hi | lo), 64 lanes, 8] of X [K, N] (input-major), N = 32 tiles; lane = 32 h + r holds
# output feature 32 tile + r.  "nat": k = 16 s + 8 h + j (the operand comes from memory); "cd": k = 16 s + 8 (j >> 2) +
# 4 h + (j & 3) (the operand is the previous MFMA's accumulator, registers 8u .. 8u+7 = k-step u).
def _frags(hi: torch.Tensor, lo: torch.Tensor, order: str) -> torch.Tensor:
    K, Nn = hi.shape
    s = torch.stack([hi, lo], 0)
    if order == "nat":                                                # (t, s, h, j, tile, r) -> (tile, s, t, h, r, j)
        return s.reshape(2, K // 16, 2, 8, Nn // 32, 32).permute(4, 1, 0, 2, 5, 3).reshape(Nn // 32, K // 16, 2, 64, 8)
    # (t, s, jh, h, jl, tile, r) -> (tile, s, t, h, r, jh, jl)
    return s.reshape(2, K // 16, 2, 2, 4, Nn // 32, 32).permute(5, 1, 0, 3, 6, 2, 4).reshape(Nn // 32, K // 16, 2, 64, 8)


def _unfrags(f: torch.Tensor, order: str) -> torch.Tensor:
    """hi + lo of `_frags` back as float64 X [K, N]."""
    tiles, ks = f.shape[0], f.shape[1]
    f = f.double()
    f = f[:, :, 0] + f[:, :, 1]                                       # (tile, s, lane, j)
    if order == "nat":                                                # (tile, s, h, r, j) -> (s, h, j, tile, r)
        return f.reshape(tiles, ks, 2, 32, 8).permute(1, 2, 4, 0, 3).reshape(16 * ks, 32 * tiles)
    # (tile, s, h, r, jh, jl) -> (s, jh, h, jl, tile, r)
    return f.reshape(tiles, ks, 2, 32, 2, 4).permute(1, 4, 2, 5, 0, 3).reshape(16 * ks, 32 * tiles)


def _by_wave(f: torch.Tensor, mt: int) -> torch.Tensor:
    """[4 mt tiles, ks, 2, 64, 8] -> rows in stream order (w, s, m, t)."""
    ks = f.shape[1]
    return f.reshape(_WAVES, mt, ks, 2, 64, 8).permute(0, 2, 1, 3, 4, 5).reshape(-1, 64, 8)


def _from_wave(rows: torch.Tensor, mt: int, ks: int) -> torch.Tensor:
    return rows.reshape(_WAVES, ks, mt, 2, 64, 8).permute(0, 2, 1, 3, 4, 5).reshape(_WAVES * mt, ks, 2, 64, 8)
