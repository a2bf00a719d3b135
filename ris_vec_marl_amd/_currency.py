"""What the host knows about theta, its candidate indices and the h_r rows of one `VecEnviron` -- and therefore which
of the RISVEC_STEP_* / RISVEC_BCD_* "this is current" bits a launch may carry.  A wrong bit makes a kernel read stale
bytes without any error, so every field behind those bits is written and read here and nowhere else: `Currency` is a
base class of `VecEnviron`, which reports events (named for what happened) and asks queries.  A base class, not a member
object, because the fields stay attributes of the env: the GPU tests assert on them there (`env._ssum_sweeps`, ...).  Pure
bookkeeping over the tensors' `_version` counters: the kernels write through raw pointers and never move a version, every
torch write does.  The class it is mixed into provides `_t` (the tensor dict), `control_bit`, `M`, `lazy_theta`,
`steer_heads`, `_theta_from_index()` (the risvec_theta_from_index launch) and `_theta_by_index_supported()`.

Invariants:
  * `_idx_valid` is only ever True with control_bit = 3 (2^b = 8 candidates): only those sweeps leave indices.
  * theta is stale (`_stale_version >= 0`: the complex64 tensor lags behind theta_idx) only after a sweep that ran by
    index, so stale implies `_idx_valid`, and it has only ever begun under lazy_theta (which may be switched off later:
    the next reader of the tensor materialises it).
  * stale excludes `_idx_current`: a by-index sweep leaves the tensor behind, a sweep that writes it ends the lag.
  * `_idx_current` (theta_idx matches tensors["theta"] AS IT IS NOW: the fused step may read either) and `_idx_valid`
    (theta_idx holds what the last sweep stored: the next sweep may start from it) are different facts.  Random_phase
    gives the first without the second; an unannounced torch write to theta takes the first (the version moves) and
    leaves the second, which only announcements and setters end.
  * `_h_r_steer_version >= 0` is only ever recorded with `_steer_valid`; `_steer_valid` alone (after a torch write to h_r,
    or a checkpoint without steer_ang) still allows steer=True, which hears announcements only.
  * a version record of -1 matches no tensor: versions start at 0.
"""
from typing import Dict, Optional

from ._native import (BCD_NO_THETA, BCD_REUSE_COLSUM, BCD_REUSE_IDX, BCD_REUSE_SSUM, STEP_H_R_STEER_CURRENT,
                      STEP_REUSE_COLSUM, STEP_REUSE_IDX, STEP_REUSE_SSUM, STEP_STEER_HEADS_CURRENT, STEP_THETA_BY_INDEX,
                      STEP_THETA_IDX_CURRENT)


class Currency:
    def _init_currency(self) -> None:
        self._eight = self.control_bit == 3    # 2^b = 8: the only candidate count with index forms
        self._chunks = self.M % 16 == 0    # rows are whole 16-element chunks: the shapes with a rebuilding kernel
        self._colsum_valid = False         # c_col matches h_r (set by compute_parms / rebuild_colsum)
        self._steer_valid = False          # h_r is the steering vector compute_parms wrote, z_r its base
        # tensors["h_r"]._version when compute_parms() last wrote it together with steer_ang (-1: never, or a checkpoint
        # without steer_ang was loaded): while it has not moved, h_r is exactly what the kernel wrote from steer_ang / z_r
        # and the fused step is told so (RISVEC_STEP_H_R_STEER_CURRENT)
        self._h_r_steer_version = -1
        # tensors["steer_ang"]._version when the chunk heads behind the angles were last written from them (-1: never)
        self._steer_head_version = -1
        self._ssum_sweeps = 0              # >0: s_sum = sum theta.c of the CURRENT theta, left by that many
                                           # consecutive sweeps (0 = unknown; refreshed every 64 sweeps)
        self._idx_valid = False            # theta_idx = candidate index of every CURRENT theta element (left by a sweep)
        # tensors["theta"]._version when the tensor went stale, i.e. began to lag behind theta_idx (-1: it does not lag).
        # A later write through torch moves the version: then the written tensor is theta (_theta_write_announced)
        self._stale_version = -1
        self._tk_ok = None                 # does the fused step have a theta-by-index form at this shape? (asked lazily)
        # tensors["theta"]._version when a kernel wrote the tensor AND the candidate index of every element of it
        # (Random_phase with control_bit = 3, or a sweep that wrote both; -1: they are not known to match): the fused step
        # may then read either, and is told so (RISVEC_STEP_THETA_IDX_CURRENT).  A write through torch moves the version
        self._idx_current_version = -1

    _theta_stale = property(lambda self: self._stale_version >= 0)
    _idx_current = property(lambda self: self._idx_current_version >= 0)

    # ------------------------------------------------------------------ events
    def _geometry_written(self) -> None:
        """compute_parms() wrote h_r, z_r, the angles and the column sums."""
        self._colsum_valid = True
        self._steer_valid = True            # h_r[e,v,m] = z_r[e,v]^m from here on
        self._h_r_steer_version = self._t["h_r"]._version
        self._ssum_sweeps = 0               # c changed: the cached sum is stale (the candidate indices are not)

    def _heads_written(self) -> None:
        """risvec_steer_heads wrote the chunk heads of the steer_ang now in the state."""
        self._steer_head_version = self._t["steer_ang"]._version

    def _colsum_rebuilt(self) -> None:
        """rebuild_colsum(): c_col matches an h_r that somebody wrote by hand."""
        self._colsum_valid = True
        self._steer_valid = False
        self._ssum_sweeps = 0

    def _h_r_write_announced(self) -> None:
        """invalidate_colsum(): h_r (and maybe theta) was written through torch."""
        self._colsum_valid = False
        self._steer_valid = False           # h_r is no longer known to be the steering vectors z_r^m
        self._theta_write_announced()

    def _theta_write_announced(self) -> None:
        """invalidate_theta(): an announced direct write that may or may not have touched theta."""
        if self._stale_version == self._t["theta"]._version:
            self._sync_theta()              # theta not written: the indices hold the swept theta, keep it
        self._theta_set(False)

    def _theta_set(self, with_idx: bool) -> None:
        """theta was written by something other than a BCD sweep: its cached sum and the sweeps' candidate indices are
        stale, and whoever wrote it made the tensor the truth again.  `with_idx`: a kernel that writes each element's
        index as well where 2^b = 8 (Random_phase)."""
        self._ssum_sweeps = 0
        self._idx_valid = False
        self._stale_version = -1
        self._idx_current_version = self._t["theta"]._version if with_idx and self._eight else -1

    def _sweep_ran(self, flags: int, step: bool) -> None:
        """A BCD sweep ran with this flag word (`step`: RISVEC_STEP_* names, in front of a fused step; else RISVEC_BCD_*)."""
        reused_s = flags & (STEP_REUSE_SSUM if step else BCD_REUSE_SSUM)
        self._colsum_valid = True
        self._ssum_sweeps = self._ssum_sweeps + 1 if reused_s else 1
        self._idx_valid = self._eight       # every 2^b = 8 sweep leaves the indices of what it stored
        version = self._t["theta"]._version
        if flags & (STEP_THETA_BY_INDEX if step else BCD_NO_THETA):
            self._stale_version, self._idx_current_version = version, -1       # it kept theta by index
        else:                              # it wrote the complex64 tensor: with 2^b = 8 it wrote both
            self._stale_version, self._idx_current_version = -1, version if self._eight else -1

    def _checkpoint_loaded(self, steer_valid: bool, h_r_steer: bool, has_steer_ang: bool) -> None:
        """load_state_dict() copied the state tensors in.  z_r travels with h_r (`_steer_valid`), and so does steer_ang,
        from the checkpoints that have it: without it the rows cannot be rebuilt until the next compute_parms() (the
        copy moved h_r's version either way).  The heads are no part of a checkpoint: a function of the angles, which the
        caller recomputes from the ones just loaded."""
        self._colsum_valid = False
        self._theta_set(False)
        self._steer_valid = steer_valid
        rebuildable = steer_valid and h_r_steer and has_steer_ang
        self._h_r_steer_version = self._t["h_r"]._version if rebuildable else -1
        self._steer_head_version = -1

    # ------------------------------------------------------------------ queries
    def _sync_theta(self) -> None:
        """Materialise tensors["theta"] from the candidate indices if the last sweeps kept theta by index."""
        if self._stale_version >= 0:
            self._theta_from_index()
            self._stale_version = -1

    def _checkpoint_record(self) -> Dict[str, bool]:
        """What state_dict() records for checkpoint_loaded()."""
        return dict(steer_valid=self._steer_valid,
                    h_r_steer=self._steer_valid and self._t["h_r"]._version == self._h_r_steer_version)

    def _sweep_flags(self, reuse_colsum: Optional[bool], step: bool) -> int:
        """The reuse bits of the next sweep.  The stand-alone sweep under lazy_theta: one that starts from the indices
        also leaves theta by index, RISVEC_BCD_NO_THETA; in front of a fused step `_fused_launch` decides."""
        reuse_c = self._colsum_valid if reuse_colsum is None else bool(reuse_colsum)
        reuse_s = reuse_c and 0 < self._ssum_sweeps < 64
        if step:
            return ((STEP_REUSE_COLSUM if reuse_c else 0) | (STEP_REUSE_SSUM if reuse_s else 0)
                    | (STEP_REUSE_IDX if self._idx_valid else 0))
        return ((BCD_REUSE_COLSUM if reuse_c else 0) | (BCD_REUSE_SSUM if reuse_s else 0)
                | ((BCD_REUSE_IDX | (BCD_NO_THETA if self.lazy_theta else 0)) if self._idx_valid else 0))     # the indices are the state

    def _idx_current_flag(self) -> int:
        """RISVEC_STEP_THETA_IDX_CURRENT while the indices are known to match the tensor: set by a kernel that wrote both,
        and nothing has written the tensor through torch since (an unannounced write moves its `_version`)."""
        return STEP_THETA_IDX_CURRENT if self._t["theta"]._version == self._idx_current_version else 0

    def _fused_launch(self, by_index: bool, current: bool) -> int:
        """THE launch-time decision of every fused RIS-cascade launch: the bits it adds to its flag word; theta is
        materialised first where the launch reads the complex64 tensor and that lags.  `by_index`: the launch has a
        theta-by-index form (step() without steer, with or without a sweep in front).  `current`: the launch takes the
        "current" bits (a plain fused step or step + store: no sweep, no steer, not the T-step launch).  The ring launch
        passes (False, True), step_many (False, False).

        Under lazy_theta no launch is told that anything is current (kept as found: the bits came after lazy_theta and
        were wired into the eager branch only), and a step() that finds theta lagging with lazy_theta switched off
        meanwhile sends none on that one launch either, while the ring does: also as found."""
        lazy = self.lazy_theta
        if lazy or self._stale_version >= 0:
            if by_index and lazy and self._idx_valid:
                if self._tk_ok is None:    # asked once: the answer depends on the shape only
                    self._tk_ok = bool(self._theta_by_index_supported())
                if self._tk_ok:
                    return STEP_THETA_BY_INDEX
            self._sync_theta()
            if lazy or by_index:
                return 0
        if not current:
            return 0
        t = self._t
        bits = STEP_THETA_IDX_CURRENT if t["theta"]._version == self._idx_current_version else 0     # _idx_current_flag()
        # RISVEC_STEP_H_R_STEER_CURRENT while h_r is known to be what compute_parms() wrote from the steer_ang / z_r now
        # in the state: nothing announced a write (rebuild_colsum / invalidate_colsum clear `_steer_valid`) and nothing
        # wrote the tensor or its complex view through torch (that moves `_version`).  Asked only at shapes whose rows are
        # whole 16-element chunks (the others have no rebuilding kernel, and a launch that is a few microseconds long
        # should not pay for the question)
        if self._chunks and self._steer_valid and t["h_r"]._version == self._h_r_steer_version:
            # ... and RISVEC_STEP_STEER_HEADS_CURRENT with it while the heads behind the angles are the angles' own:
            # written since (compute_parms / load_state_dict), and no torch write has moved the angles' version since
            if self.steer_heads and t["steer_ang"]._version == self._steer_head_version:
                return bits | STEP_H_R_STEER_CURRENT | STEP_STEER_HEADS_CURRENT
            return bits | STEP_H_R_STEER_CURRENT
        return bits
