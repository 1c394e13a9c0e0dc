"""What per-tile ordered-dither levels of a shared-palette set (snesimage_shared_level_sweep, DESIGN 5d'') cost and gain, tied and
per frame: sets of 2, 4 and 8 frames of 256 x 224 (synth_image, one seed per frame), 8 x 15, RGB, Bayer 4 x 4 at amplitude 32, a
ladder of four levels, one MI355X.

    python profiles/set_tile_dither.py [--calls 2400] [--frames 2,4,8] [--levels 4] [--out profiles/set_tile_dither.json]

Every set is a child process of its own under a time limit (a child that fails ends the run: nothing more is started on the
device).  A child forms the set, gives it the bank with every tile on the full amplitude, runs the set's initialisers and `--calls`
calls of the reference's loop (snesimage_shared_run_slots), and keeps that state.  From that state, put back before every leg
(the palette, every member's levels), it times one level sweep over all 896 tile positions for each of tied / per frame x
window 0 / window 1, by the host clock around the synchronous call after an untimed sweep over the first 64 tiles has sized
the workspaces -> windows per second, calls accepted, E before and after; and reports E of the tied result against the
per-frame result and, under `frame`, how many tile positions end on different levels in different frames.
The output is stamped with the library's source hash."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 224


def child(a):
    sys.path.insert(0, ROOT)
    import numpy as np
    import snesimage_amd as S
    from snesimage_amd import _ffi
    from snesimage_amd.synth import synth_image
    F, L = a.set, a.levels
    bank = np.stack([np.zeros((4, 4), np.int8)] + [S.bayer_offsets(4, a.amplitude * j // (L - 1)) for j in range(1, L)])
    ctxs = [S.OptimizedImage(synth_image(0x5EED7000 + i, 256, H), 8, 15) for i in range(F)]
    for c in ctxs:
        c.set_ordered_dither(bank[L - 1])
        c.set_chunk(64)
    sp = S.SharedPalette(ctxs)
    sp.set_ordered_dither_bank(bank, L - 1)
    sp.initialize_tiles()
    sp.recalculate_palettes()
    out = {"frames": F, "levels": L, "calls": a.calls, "version": _ffi.load().snesimage_version().decode(), "error_start": sp.error()}
    t0 = time.perf_counter()
    sp.run_slots(a.calls, seed=1, want_log=False)
    out["run_s"] = time.perf_counter() - t0
    pal, ntile = sp.palette, 32 * (H // 8)
    start = np.zeros(1024, np.uint8)
    start[:ntile] = L - 1

    def reset():
        sp.palette = pal
        for i in range(F):
            sp.set_tile_levels(i, start)
        return sp.error()
    for tied in (True, False):
        for window in (0, 1):
            reset()
            sp.level_sweep(0, 64, window=window, tied=tied)  # sizes the workspaces
            e0 = reset()
            t0 = time.perf_counter()
            _, st = sp.level_sweep(window=window, tied=tied)
            dt = time.perf_counter() - t0
            leg = {"seconds": dt, "windows": st["windows"], "windows_per_s": st["windows"] / dt, "calls": st["calls"], "accepted": st["accepted"], "scored": st["scored"],
                   "E_before": e0, "E_after": sp.error()}
            if not tied:
                lv = sp.tile_levels[:, :ntile]
                leg["positions_on_different_levels"] = int((lv != lv[0]).any(0).sum())
            leg["tiles_per_level"] = [int((sp.tile_levels[:, :ntile] == l).sum()) for l in range(L)]
            out["%s_w%d" % ("tied" if tied else "frame", window)] = leg
    out["E_tied_minus_frame"] = out["tied_w0"]["E_after"] - out["frame_w0"]["E_after"]
    print(json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2400)
    ap.add_argument("--frames", default="2,4,8")
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--amplitude", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_tile_dither.json"))
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--set", type=int, default=2)
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"runs": []}
    for F in [int(x) for x in a.frames.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--set", str(F), "--calls", str(a.calls), "--levels", str(a.levels), "--amplitude", str(a.amplitude)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            print(json.dumps({"failed": cmd[2:], "rc": r.returncode, "stderr": r.stderr[-600:]}), flush=True)
            return 1
        run = json.loads(r.stdout.strip().splitlines()[-1])
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
    res["library"] = res["runs"][0]["version"]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
