"""The model of a backdrop set (snesimage_shared_create_backdrop; DESIGN 5c'') over the unchanged CPU oracle.

One backdrop_model.Model per member: the oracle's expanded context (C, S + 1) whose column S holds the set's B.  The tied
call sums the members' `tied_candidates` in member order, regular calls sum `score_candidates` on the expanded contexts; the
acceptance rule is test_shared_palette.py's (strict < against the summed incumbents, NES takes the argmin, the lowest k wins
ties); the schedule is backdrop_model.model_schedule.  The initialisers are the stacked oracle's at (C, S).  CPU only."""
import numpy as np

import backdrop_model as M

REL = M.REL_ERR
ALPHA_H = 104  # the smallest height at which variant 1's transparent square, rows 96 .. 159, shows (8 rows of it)


def frames(F, H, variant=0, seed=0x5EED5B00):
    from snesimage_amd.synth import synth_image
    return [synth_image(seed + i, 256, H, variant) for i in range(F)]


def creation_frames(F=3):
    """Frames with the transparent square whose own means differ (member 1 with half its red, member 2 with its blue turned
    round), so that the mean of the stack is no member's own."""
    imgs = frames(F, ALPHA_H, 1)
    if F > 1:
        imgs[1][..., 0] //= 2
    if F > 2:
        imgs[2][..., 2] = 255 - imgs[2][..., 2]
    return imgs


def stack_backdrop(O, imgs, flags):
    """B as snesimage_shared_create_backdrop sets it: snesimage_create's rule over the opaque pixels of all members."""
    return M.mean_backdrop(np.concatenate(imgs, axis=0), O, bool(flags.get("nes")), bool(flags.get("perceptual")))


def stack_backdrop_by_hand(imgs):
    """The same without the concatenated picture: the channel sums and the count added member after member."""
    s, n = [0, 0, 0], 0
    for img in imgs:
        opaque = img[..., 3] != 0
        n += int(opaque.sum())
        for c in range(3):
            s[c] += int(img[..., c][opaque].astype(np.int64).sum())
    if n == 0:
        return np.zeros(3, np.uint8)
    return np.array([((s[c] + n // 2) // n) >> 3 for c in range(3)], np.uint8)


class SetModel:
    def __init__(self, O, imgs, C, S, flags, B=None, init=True):
        self.O, self.C, self.S, self.flags, self.imgs = O, C, S, dict(flags), imgs
        H = imgs[0].shape[0]
        self.per = 32 * (H // 8)  # tiles per member
        self.m = [M.Model(O, img, C, S, flags, init="zero") for img in imgs]
        self.B = stack_backdrop(O, imgs, flags) if B is None else np.array(B, np.uint8)
        self.set_state(np.zeros((C * S, 3), np.uint8), self.B)
        if init:
            self.initialize()

    def close(self):
        for m in self.m:
            m.o.close()

    def initialize(self):
        """initialize_tiles + recalculate_palettes of the stacked oracle at (C, S); B is not an initialiser's to move."""
        st = self.O.OracleImage(np.concatenate(self.imgs, axis=0), self.C, self.S, **self.flags)
        st.initialize_tiles()
        self.tiles_after_init, self.regular_after_init = self.split_tiles(st.tile_palettes), st.palette
        st.recalculate_palettes()
        self.set_tiles(self.split_tiles(st.tile_palettes))
        self.set_state(st.palette, self.B)
        st.close()

    def split_tiles(self, tp):
        out = []
        for i in range(len(self.m)):
            t = np.zeros(1024, np.uint8)
            t[:self.per] = tp[i * self.per:(i + 1) * self.per]
            out.append(t)
        return out

    def set_tiles(self, tiles):
        for m, t in zip(self.m, tiles):
            m.o.tile_palettes = t

    def set_state(self, regular, B):
        self.B = np.array(B, np.uint8)
        for m in self.m:
            m.set_state(regular, B)

    @property
    def regular(self):
        return self.m[0].regular

    def error(self):
        E = 0.0
        for m in self.m:
            E = E + m.error()
        return E

    # -- scores: the members' summed in member order --------------------------------------------------------------------
    def tied_candidates(self, cand):
        E = None
        for m in self.m:
            e = m.tied_candidates(cand)
            E = e if E is None else E + e
        return E

    def score_candidates(self, p, i, cand):
        if p == self.C:
            return self.tied_candidates(cand)
        E = None
        for m in self.m:
            e = m.o.score_candidates(p, i, cand)
            E = e if E is None else E + e
        return E

    # -- one scheduled call -------------------------------------------------------------------------------------------------
    def candidates(self, method, p, i, ch, seed, step_id, n_random):
        if method == 0:
            return self.O.random_candidates(seed, step_id, n_random or 64)
        if method == 1:
            cur = self.B if p == self.C else self.m[0].o.palette[p * (self.S + 1) + i]
            cand = np.repeat(np.array(cur, np.uint8)[None, :], 32, 0)
            cand[:, ch] = np.arange(32)
            return cand
        return np.array([self.O.nes_color(k) for k in range(56)], np.uint8)

    def call(self, method, p, i, ch, seed, step_id, n_random=0, guard=True):
        """-> (E after, best_k, the slot's colour after, changed, tied)"""
        cand = self.candidates(method, p, i, ch, seed, step_id, n_random)
        inc = self.error()
        E = self.score_candidates(p, i, cand)
        best, best_k = (inc, -1) if method != 2 else (float("inf"), -1)
        for k, e in enumerate(E):
            if guard and np.isfinite(best):
                M.check_gap(e, best)
            if e < best:
                best, best_k = e, k
        took = best_k >= 0
        if method == 2 and best_k < 0:
            best_k = 0
        tied = p == self.C
        before = self.B.copy() if tied else self.m[0].o.palette[p * (self.S + 1) + i].copy()
        after = before
        if best_k >= 0:
            after = cand[best_k].copy()
            if tied:
                self.set_state(self.regular, after)
            else:
                reg = self.regular
                reg[p * self.S + i] = after
                self.set_state(reg, self.B)
        else:
            for m in self.m:
                m.o.optimize()  # lib.rs:237
        return (best if took else inc), (best_k if took or method == 2 else -1), after, int(not np.array_equal(after, before)), tied


def trajectory(O, imgs, C, S, flags, n_calls, seed, state=(0, 0, 0, 0), n_random=16, guard=True, B0=None):
    """The model's run -> (model, records, final scheduler state); step_id of call j is j."""
    nes = bool(flags.get("nes"))
    sm = SetModel(O, imgs, C, S, flags)
    if B0 is not None:
        sm.set_state(sm.regular, B0)
    sched_all = M.model_schedule(O, C, S, 6 * (C * S + 1) * 3 + n_calls + 8, nes)
    start = next(k for k, r in enumerate(sched_all) if r[1:] == tuple(state))
    recs = []
    for j in range(n_calls):
        method, p, i, ch, st = sched_all[start + j]
        e, k, rgb, changed, tied = sm.call(method, p, i, ch, seed, j, n_random if method == 0 else 0, guard)
        recs.append(dict(method=method, p=p, i=i, ch=ch, error=e, best_k=k, rgb5=np.array(rgb), changed=changed, tied=tied, accepted=k >= 0 and (method != 2 or changed),
                         regular=sm.regular, B=sm.B.copy(), pmaps=[m.palette_map for m in sm.m]))
    return sm, recs, sched_all[start + n_calls][1:]


# The trajectories the GPU tests follow (tests/test_set_backdrop.py): F = 2 frames of 256x32, (C, S) = (2, 3), 16 random
# candidates.  Seeds and start colours were chosen on the CPU so that the gap premise holds and at least one backdrop call
# accepts and one rejects; tests/test_set_backdrop_model.py proves both on every run.
#         flags, n_calls, seed, scheduler state, B0 (None: the stack mean)
TRAJ = {
    "rgb": ({}, 35, 3, (0, 0, 0, 3), None),
    "dither": (dict(dither=True), 35, 1, (0, 0, 0, 3), None),
    "nes": (dict(nes=True), 14, 1, (0, 0, 0, 0), [19, 6, 0]),  # nes_color(20): a table colour that is not the argmin
}
TRAJ_F, TRAJ_H, TRAJ_GEOM, N_RANDOM = 2, 32, (2, 3), 16
_runs = {}


def traj_run(O, name):
    """(model, records, final state) of TRAJ[name], computed once per process."""
    if name not in _runs:
        flags, n, seed, state, B0 = TRAJ[name]
        _runs[name] = trajectory(O, frames(TRAJ_F, TRAJ_H), TRAJ_GEOM[0], TRAJ_GEOM[1], flags, n, seed, state, N_RANDOM, True, B0)
    return _runs[name]
