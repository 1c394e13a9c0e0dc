"""Guided calls of a set through the slot windows (include/snesimage_hip.h: snesimage_shared_guided_run_slots; DESIGN 5f'''').

The semantics are set_guided_model.SetModel.sweep(K, n): there is no new arithmetic in the decisions.  This file holds the inputs —
the six set_guided_model.CASES, run for three sweeps from the stacked k-means start — and the decisions recorded from the model on
the CPU; tests/test_set_guided_window_model.py recomputes them with the gap guard on and asserts them, and with them the premises
the GPU tests (tests/test_set_guided_windows.py) rest on: windows that void calls, clean windows, and windows that hold one slot
twice.  It also holds the identity the windows' generator rests on, in numpy integers: one table per subpalette plus one
correction per call (window_costs).  Everything here runs on the CPU."""
import numpy as np

import guided_model as GM
import set_guided_model as SGM

SWEEPS = 3

# name -> '1' where the call changed the palette, in call order over the three sweeps
CHANGED = {
    "plain-f2-2x3": "111011000000000000",
    "plain-f3-2x3": "111011101111000000",
    "perceptual-f2-2x3": "010111100000000000",
    "dither-f2-2x3": "111111011101000000",
    "backdrop-f2-2x3": "111011101110111001011",
    "plain-f2-4x7": "011111101111001011101111111111100010100100111100010001000000000011010000000001000001",
}


def slots(name):
    """The guided sweep's slot order for the case: index inner, palette outer, the tied slot of a backdrop set last."""
    F, H, C, S, flags, B0, K, n = SGM.CASES[name]
    return [(p, i) for p in range(C) for i in range(S)] + ([(C, 0)] if B0 is not None else [])


def n_calls(name):
    return SWEEPS * len(slots(name))


_runs = {}


def run(O, name):
    """The model's three sweeps on the case, computed once with the gap guard on -> (records, smallest non-zero gap)."""
    if name not in _runs:
        m = SGM.case_model(O, name)
        recs = m.sweep(SGM.CASES[name][6], n_calls(name), guard=True)
        _runs[name] = ([dict(p=r["p"], i=r["i"], error=r["error"], best_k=r["best_k"], rgb5=r["rgb5"], changed=r["changed"]) for r in recs], m.min_gap)
        m.close()
    return _runs[name]


def kmax(name, window_max=64):
    """Calls a window of the case's set may hold: F slot contexts per call, SNES_WINDOW_MAX (default 64) in all."""
    return window_max // SGM.CASES[name][0]


def consume(name, window):
    """How snesimage_shared_guided_run_slots at a fixed `window` walks the case's recorded decisions -> a list of launch sets
    dict(first, taken, used, accepted): a window takes the next `window` calls (at most kmax) but ends in front of the tied
    slot, which is a launch set of its own; it takes effect up to and including its first accepting call."""
    seq, sl = CHANGED[name], slots(name)
    window = min(window, kmax(name))
    tied = SGM.CASES[name][5] is not None
    out, at = [], 0
    while at < len(seq):
        taken = 0
        if tied and at % len(sl) == len(sl) - 1:
            taken = 1
        else:
            while taken < window and at + taken < len(seq) and not (tied and (at + taken) % len(sl) == len(sl) - 1):
                taken += 1
        hit = seq.find("1", at, at + taken)
        used = taken if hit < 0 else hit - at + 1
        out.append(dict(first=at, taken=taken, used=used, accepted=int(hit >= 0)))
        at += used
    return out


# ---- the generator's identity ------------------------------------------------------------------------------------------------

def population(Ts, tiles, p):
    """The opaque pixels of every tile of every member on subpalette p -> rgb8 (n, 3), as guided_model.costs reads them."""
    out = []
    for T, tp in zip(Ts, tiles):
        T = np.asarray(T)
        for t in range(32 * (T.shape[0] // 8)):
            if tp[t] == p:
                blk = T[(t // 32) * 8:(t // 32) * 8 + 8, (t % 32) * 8:(t % 32) * 8 + 8].reshape(64, 4)
                out.append(blk[blk[:, 3] != 0, :3])
    return np.concatenate(out) if out else np.zeros((0, 3), np.uint8)


def window_costs(Ts, tiles, internal, Si, p):
    """(A_p, [D_{p,i} for i in range(Si)]) in integers: with a(x) the lowest key of pixel x over the Si entries of subpalette p,
    j*(x) the first entry that reaches it and b(x) the lowest key over j != j*(x) (0xFFFFFFFF with one entry),
    A_p(u) = sum min(a, key(x, u)) and D_{p,i}(u) = sum over j* == i of min(b, key(x, u)) - min(a, key(x, u))."""
    A, D = np.zeros(GM.NCOL, np.uint64), [np.zeros(GM.NCOL, np.uint64) for _ in range(Si)]
    px = population(Ts, tiles, p)
    if len(px) == 0:
        return A, D
    px, cnt = np.unique(px, axis=0, return_counts=True)  # a, b and j* depend on the pixel's colour only
    ent = GM.expand5(np.asarray(internal).reshape(-1, 3)[p * Si:(p + 1) * Si])
    keys = np.stack([GM.red_mean_key(px, e) for e in ent], axis=1)  # (n, Si) int64
    js = keys.argmin(axis=1)  # the first entry that reaches the minimum
    a = keys[np.arange(len(px)), js]
    rest = keys.copy()
    rest[np.arange(len(px)), js] = GM.NO_FLOOR
    b = rest.min(axis=1)
    allc = GM.expand5(GM.unpack_u(np.arange(GM.NCOL)))  # (32768, 3)
    w = cnt.astype(np.int64)
    for lo in range(0, len(px), 128):
        s = slice(lo, lo + 128)
        ku = GM.red_mean_key(px[s, None, :], allc[None, :, :])  # (chunk, 32768)
        ma = np.minimum(ku, a[s, None])
        A += (ma * w[s, None]).sum(axis=0).astype(np.uint64)
        mb = (np.minimum(ku, b[s, None]) - ma) * w[s, None]
        assert (mb >= 0).all()
        for i in range(Si):
            sel = js[s] == i
            if sel.any():
                D[i] += mb[sel].sum(axis=0).astype(np.uint64)
    return A, D
