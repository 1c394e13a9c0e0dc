"""Guided calls through the slot windows (include/snesimage_hip.h: snesimage_guided_run_slots; DESIGN 5f''').

The semantics are guided_model.Model.sweep(K, n): there is no new arithmetic.  This file holds the inputs — the five
guided_model.CASES, run for three sweeps from the k-means start — and the decisions recorded from the model on the CPU;
tests/test_guided_window_model.py recomputes them with the gap guard on and asserts them, and with them the premises the GPU
tests (tests/test_guided_windows.py) rest on: windows that void calls, clean windows, and a window enqueued ahead that the
device voids.  Everything here runs on the CPU."""
import guided_model as GM

SWEEPS = 3

# name -> '1' where the call changed the palette, in call order over the three sweeps
CHANGED = {
    "plain-2x3": "111111000110101000",
    "dither-2x3": "111111010110000000",
    "perceptual-2x3": "111100100000000000",
    "backdrop-2x3": "011110010000000000000",
    "plain-4x7": "111001111111111111111111111111111010110101001000011111011010000010110100000000100001",
}


def slots(name):
    """The guided sweep's slot order for the case: index inner, palette outer, the tied slot of a backdrop context last."""
    h, seed, C, S, flags, backdrop, K, n = GM.CASES[name]
    return [(p, i) for p in range(C) for i in range(S)] + ([(C, 0)] if backdrop else [])


def n_calls(name):
    return SWEEPS * len(slots(name))


_runs = {}


def run(O, name):
    """The model's three sweeps on the case, computed once with the gap guard on -> (records, smallest non-zero gap)."""
    if name not in _runs:
        m = GM.case_model(O, name)
        recs = m.sweep(GM.CASES[name][6], n_calls(name), guard=True)
        _runs[name] = ([dict(p=r["p"], i=r["i"], error=r["error"], best_k=r["best_k"], rgb5=r["rgb5"], changed=r["changed"]) for r in recs], m.min_gap)
        m.close()
    return _runs[name]


def consume(name, window):
    """How snesimage_guided_run_slots at a fixed `window` walks the case's recorded decisions -> a list of launch sets
    dict(first, taken, used, accepted): a window takes the next `window` calls but ends in front of the tied slot, which is a
    launch set of its own; it takes effect up to and including its first accepting call."""
    seq, sl = CHANGED[name], slots(name)
    tied = GM.CASES[name][5]
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
