"""The case table of the mobility tests (plain NumPy, no GPU, no test collection): vehicle states placed ON the branches
and equality edges of one `renew_positions()` move (`k_mobility` in csrc/k_env.hip, `oracle.risvec_oracle.mobility`).

The golden captures and the Philox rollout of tests/test_hip_parity.py drive every vehicle at 10-14 m/s with time_slow =
0.1, so a move crosses at most one lane and consumes at most one turn draw.  Here a move may cross every lane of both
lists (8 draws at time_slow = 20), starts on a lane, lands on one exactly, turns onto a lane outside the map, leaves the
map straight or right after a turn, and meets the float32 draw 0.4 itself.

`walk()` restates one vehicle's move with the statements of `orc.mobility`, in their order, and names every branch it
takes; `expected_ids()` is the table of names a case set must reach; `case_sets()` builds the sets; `philox_case()` is the
state whose draws are the kernel's own.  tests/test_mobility_cases_host.py checks all of this against the oracle,
tests/test_env_kernels_hip.py runs the sets on the device.

Branch names:
    <dir>/<first|second>/<j>/<pass|turn>     the draw of lane j of the first / second lane list this direction looks at
                                             (U, D: left then right lanes; R, L: up then down lanes) was >= 0.4 / < 0.4
    <dir>/<first|second>/<j>/at-lane         that crossing was detected with the coordinate ON the lane before the move
    <dir>/<first|second>/<j>/lands-on-lane   ... with coordinate +- dd == lane exactly
    <dir>/straight                           no turn: the vehicle advanced by dd
    exit/<straight|after-turn>/<dir>         the vehicle left the map, heading <dir> when it did (the branch of the exit
                                             handling that ran), without / right after a turn
    draws/<k>                                the move consumed k draws
"""
from typing import Dict, FrozenSet, List, Sequence, Tuple

import numpy as np

from oracle import risvec_oracle as orc

DIR_NAMES = {orc.DIR_U: "U", orc.DIR_D: "D", orc.DIR_L: "L", orc.DIR_R: "R"}
VELOCITIES = np.array([10, 12, 13.25, 14, 15, 17.5, 19], dtype=np.float32)
# 0.4f is 0.4000000059 as a double: it does NOT turn; its float32 predecessor does.  No draw is merely "near" 0.4.
DRAWS = np.array([0.1, 0.9, 0.4, np.nextafter(np.float32(0.4), np.float32(0))], dtype=np.float32)
PASSING = DRAWS[[1, 2]]
PLACEMENTS = ("on-lane", "dd-before-lane", "inside-dd-of-lane", "over-the-map", "at-the-border", "just-past-lane")
N_STATES = 6300           # divisible by 4, 6 and 7 (the vehicle counts the device test uses), no multiple of 256
N_STATES_ONE_LANE = 3360


def _note(ids: List[str], dname: str, fam: str, j: int, coord: float, landed: float, lane: float, u: float) -> None:
    pre = "%s/%s/%d/" % (dname, fam, j)
    ids.append(pre + ("turn" if u < 0.4 else "pass"))
    if coord == lane:
        ids.append(pre + "at-lane")
    if landed == lane:
        ids.append(pre + "lands-on-lane")


def walk(x: float, y: float, d: int, vel: float, u_row: Sequence[float], lanes: Dict[str, Sequence[float]], width: float,
         height: float, time_slow: float) -> Tuple[float, float, int, int, List[str]]:
    """One vehicle's move in float64: (x, y, dir, n_used, branch names).  vel and u_row are the float64 images of the
    float32 values the device holds."""
    DIR_U, DIR_D, DIR_L, DIR_R = orc.DIR_U, orc.DIR_D, orc.DIR_L, orc.DIR_R
    x, y, d, vel = float(x), float(y), int(d), float(vel)
    up, down, left, right = (list(lanes[k]) for k in ("up", "down", "left", "right"))
    ids: List[str] = []
    dd = vel * time_slow
    turned = False
    nd = 0
    if d == DIR_U:
        for j, lane in enumerate(left):
            if y <= lane and (y + dd) >= lane:
                u = float(u_row[nd]); nd += 1
                _note(ids, "U", "first", j, y, y + dd, lane, u)
                if u < 0.4:
                    x, y, d, turned = x - (dd - (lane - y)), lane, DIR_L, True
                    break
        if not turned:
            for j, lane in enumerate(right):
                if y <= lane and (y + dd) >= lane:
                    u = float(u_row[nd]); nd += 1
                    _note(ids, "U", "second", j, y, y + dd, lane, u)
                    if u < 0.4:
                        x, y, d, turned = x + (dd + (lane - y)), lane, DIR_R, True
                        break
        if not turned:
            y += dd
            ids.append("U/straight")
    if d == DIR_D and not turned:
        for j, lane in enumerate(left):
            if y >= lane and (y - dd) <= lane:
                u = float(u_row[nd]); nd += 1
                _note(ids, "D", "first", j, y, y - dd, lane, u)
                if u < 0.4:
                    x, y, d, turned = x - (dd - (y - lane)), lane, DIR_L, True
                    break
        if not turned:
            for j, lane in enumerate(right):
                if y >= lane and (y - dd) <= lane:
                    u = float(u_row[nd]); nd += 1
                    _note(ids, "D", "second", j, y, y - dd, lane, u)
                    if u < 0.4:
                        x, y, d, turned = x + (dd + (y - lane)), lane, DIR_R, True
                        break
        if not turned:
            y -= dd
            ids.append("D/straight")
    if d == DIR_R and not turned:
        for j, lane in enumerate(up):
            if x <= lane and (x + dd) >= lane:
                u = float(u_row[nd]); nd += 1
                _note(ids, "R", "first", j, x, x + dd, lane, u)
                if u < 0.4:
                    x, y, d, turned = lane, y + (dd - (lane - x)), DIR_U, True
                    break
        if not turned:
            for j, lane in enumerate(down):
                if x <= lane and (x + dd) >= lane:
                    u = float(u_row[nd]); nd += 1
                    _note(ids, "R", "second", j, x, x + dd, lane, u)
                    if u < 0.4:
                        x, y, d, turned = lane, y - (dd - (lane - x)), DIR_D, True
                        break
        if not turned:
            x += dd
            ids.append("R/straight")
    if d == DIR_L and not turned:
        for j, lane in enumerate(up):
            if x >= lane and (x - dd) <= lane:
                u = float(u_row[nd]); nd += 1
                _note(ids, "L", "first", j, x, x - dd, lane, u)
                if u < 0.4:
                    x, y, d, turned = lane, y + (dd - (x - lane)), DIR_U, True
                    break
        if not turned:
            for j, lane in enumerate(down):
                if x >= lane and (x - dd) <= lane:
                    u = float(u_row[nd]); nd += 1
                    _note(ids, "L", "second", j, x, x - dd, lane, u)
                    if u < 0.4:
                        x, y, d, turned = lane, y - (dd - (x - lane)), DIR_D, True
                        break
            if not turned:
                x -= dd
                ids.append("L/straight")
    if x < 0 or y < 0 or x > width or y > height:
        ids.append("exit/%s/%s" % ("after-turn" if turned else "straight", DIR_NAMES[d]))
        if d == DIR_U:
            d, y = DIR_R, right[-1]
        elif d == DIR_D:
            d, y = DIR_L, left[0]
        elif d == DIR_L:
            d, x = DIR_U, up[0]
        elif d == DIR_R:
            d, x = DIR_D, down[-1]
    ids.append("draws/%d" % nd)
    return x, y, d, nd, ids


def walk_all(lanes, width, height, time_slow, pos, direc, vel, u_turn):
    """`walk` over a flat set of states: (pos [n,2], dir [n], n_used [n], the set of branch names reached)."""
    n = direc.shape[0]
    out_pos, out_dir, out_nd, seen = np.zeros((n, 2)), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), set()
    v64, u64 = vel.astype(np.float64), u_turn.astype(np.float64)
    for i in range(n):
        x, y, d, nd, ids = walk(pos[i, 0], pos[i, 1], direc[i], v64[i], u64[i], lanes, width, height, time_slow)
        out_pos[i], out_dir[i], out_nd[i] = (x, y), d, nd
        seen.update(ids)
    return out_pos, out_dir, out_nd, seen


def expected_ids(n_lanes: int, max_draws: int) -> FrozenSet[str]:
    """Every branch name a set with `n_lanes` lanes per list can reach when one move consumes up to `max_draws` draws."""
    ids = set()
    for dname in "UDLR":
        for fam in ("first", "second"):
            for j in range(n_lanes):
                ids.update("%s/%s/%d/%s" % (dname, fam, j, k) for k in ("pass", "turn", "at-lane", "lands-on-lane"))
        ids.update(("%s/straight" % dname, "exit/straight/%s" % dname, "exit/after-turn/%s" % dname))
    ids.update("draws/%d" % k for k in range(max_draws + 1))
    return frozenset(ids)


# ---------------------------------------------------------------------------- the builders
def _build(lanes, width, height, time_slow, n, seed):
    """n states, each aimed at one (direction, lane list, lane, placement): see PLACEMENTS.  Deterministic in `seed`."""
    rng = np.random.default_rng(seed)
    n_lanes = len(lanes["up"])
    pos, direc = np.zeros((n, 2)), np.zeros(n, dtype=np.int64)
    vel = VELOCITIES[rng.integers(0, len(VELOCITIES), n)]
    # a vehicle's first k draws pass (k = 0...8), the rest are any of the four: deep draws are as common as shallow ones
    u_turn = DRAWS[rng.integers(0, len(DRAWS), (n, 8))]
    prefix = rng.integers(0, 9, n)
    passing = PASSING[rng.integers(0, len(PASSING), (n, 8))]
    u_turn = np.where(np.arange(8)[None, :] < prefix[:, None], passing, u_turn).astype(np.float32)
    for i in range(n):
        d = int(rng.integers(0, 4))
        fam, j, place = int(rng.integers(0, 2)), int(rng.integers(0, n_lanes)), int(rng.integers(0, len(PLACEMENTS)))
        vertical = d in (orc.DIR_U, orc.DIR_D)
        names = ("left", "right") if vertical else ("up", "down")
        lane = float(lanes[names[fam]][j])
        s = 1.0 if d in (orc.DIR_U, orc.DIR_R) else -1.0                    # the coordinate grows / shrinks
        along_max, cross_max = (height, width) if vertical else (width, height)
        dd = float(vel[i]) * time_slow
        if place == 0:
            a = lane
        elif place == 1:
            a = lane - s * dd
        elif place == 2:
            a = lane - s * dd * rng.uniform(0.0, 1.0)
        elif place == 3:
            a = rng.uniform(-1.0, along_max + 1.0)
        elif place == 4:
            a = (along_max if s > 0 else 0.0) - s * dd * rng.uniform(0.0, 1.0)
        else:
            a = float(np.nextafter(lane, s * np.inf)) if rng.integers(0, 2) else lane + s * rng.uniform(0.0, 0.5)
        kind = rng.uniform()
        if kind < 0.4:
            c = rng.uniform(-1.0, cross_max + 1.0)
        elif kind < 0.7:
            c = rng.uniform(-0.5, 1.0) if time_slow < 1 else rng.uniform(-0.5, 100.0)
        else:
            c = cross_max - (rng.uniform(-0.5, 1.0) if time_slow < 1 else rng.uniform(-0.5, 100.0))
        pos[i] = (c, a) if vertical else (a, c)
        direc[i] = d
    return dict(lanes), float(width), float(height), float(time_slow), pos, direc, vel, u_turn


def reference_set(time_slow: float, n: int = N_STATES):
    """The reference driver's lanes on its 400 x 400 map: the second cluster of the up / left lists (400.875, 402.625)
    lies outside the map, so a turn onto it is followed by the exit handling at once."""
    return _build(orc.default_lanes(), 400, 400, time_slow, n, seed=int(round(time_slow * 1000)))


DYADIC_LANES = dict(up=[100.5, 102.25], down=[97.0, 98.75], left=[150.5, 152.25], right=[147.0, 148.75])


def dyadic_set(n: int = N_STATES):
    """Two lanes per list, every coordinate a short dyadic number, time_slow = 0.125 on 300 x 500: vel * 0.125 is exact, so
    `lands-on-lane` is an exact float equality and not a matter of rounding."""
    return _build(DYADIC_LANES, 300, 500, 0.125, n, seed=125)


ONE_LANE = dict(up=[101.0], down=[99.5], left=[101.0], right=[99.5])


def one_lane_set(n: int = N_STATES_ONE_LANE):
    """One lane per list on 200 x 200 at time_slow = 0.1: lanes_x[n_lanes - 1] of the exit handling is lanes_x[0]."""
    return _build(ONE_LANE, 200, 200, 0.1, n, seed=1)


# name -> (builder, vehicles per env in the device test, the branch names the set must reach).  Draws per move: the
# reference lanes of one axis are 1.75 m apart in two clusters (196.375-202.625 and 396.375-402.625); dd <= 1.9 m at
# time_slow 0.1 spans two lanes, <= 9.5 m at 0.5 one cluster (4), >= 240 m at 20 both (8).  Dyadic set: dd <= 2.375 m,
# lanes 1.75 m apart: 2.  One-lane set: the two lanes a direction looks at are 1.5 m apart, dd <= 1.9 m: 2.
SETS = {
    "ref_0.1": (lambda: reference_set(0.1), 4, expected_ids(4, 2)),
    "ref_0.5": (lambda: reference_set(0.5), 6, expected_ids(4, 4)),
    "ref_20": (lambda: reference_set(20.0), 7, expected_ids(4, 8)),
    "dyadic": (dyadic_set, 6, expected_ids(2, 2)),
    "one_lane": (one_lane_set, 7, expected_ids(1, 2)),
}


# ---------------------------------------------------------------------------- the Philox case
PHILOX_E, PHILOX_V, PHILOX_SEED = 512, 8, 5
PHILOX_OFFSETS = (0, 2 ** 31 - 3)


def philox_case():
    """(lanes, width, height, time_slow, pos [E,V,2], dir [E,V], vel [E,V] float32): the reference lanes on a 500 x 500 map
    (both lane clusters inside it) at time_slow = 20, U and R vehicles at 190 and D and L vehicles at 410 along their axis:
    dd >= 240 m takes every vehicle across all eight lanes of its two lists, so a move consumes draws until one turns."""
    E, V = PHILOX_E, PHILOX_V
    direc = np.tile(np.array([orc.DIR_U, orc.DIR_D, orc.DIR_L, orc.DIR_R], dtype=np.int64), (E, V // 4))
    vel = np.tile(np.array([12, 13.25, 14, 12, 14, 12, 13.25, 14], dtype=np.float32), (E, 1))
    along = np.where((direc == orc.DIR_U) | (direc == orc.DIR_R), 190.0, 410.0)
    vertical = (direc == orc.DIR_U) | (direc == orc.DIR_D)
    pos = np.where(vertical[..., None], np.stack([np.full((E, V), 250.0), along], -1), np.stack([along, np.full((E, V), 250.0)], -1))
    return orc.default_lanes(), 500.0, 500.0, 20.0, pos, direc, vel
