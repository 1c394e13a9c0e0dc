"""What a refit sweep across the members of a shared-palette set (snesimage_shared_refit_characters, DESIGN 5e''') costs and what
it wins back behind the set's character reduction: frames of 256 x 224 (896 tiles each), 8 x 15, RGB, one MI355X.

    python profiles/set_refit.py [--frames 2,4,8] [--calls 240] [--shortlist 16] [--steps 24] [--sweeps 3] [--out FILE]

The leg `joint` forms a set of F frames (the bench image's generator, one seed per frame), starts from the set's k-means
initialisers, runs `--calls` calls of the reference's loop through snesimage_shared_run_slots, reduces the set to
N = (U0 - F * `--steps`) rounded down to a multiple of F with snesimage_shared_reduce_characters, and then runs up to `--sweeps`
refit sweeps (it stops after one that accepts nothing).  Per sweep, with the host clock around the synchronous call: wall_ms,
calls / accepted / skipped, windows, the calls whose accepted refit spans more than one member, E before and after, U.
`fits_ms` is snesimage_shared_character_fits (characters, classes, the fit kernel and the copy back; mean of 3 after 1): an upper
bound of the fit's share of a sweep.
The leg `separate` gives every frame a context of its own with the set's palette and tile palettes, reduces it to N / F with
snesimage_reduce_characters and refits it with snesimage_refit_characters (as many sweeps at most): the sum of the members'
errors after the reduction alone and after reduction + refit, and the characters the frames hold when counted together.
Every measurement is a child process of its own under a time limit; a child that fails ends the run: nothing more is started
on the device.  The output is stamped with the library's source hash."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def child(a):
    sys.path.insert(0, a.root)
    import numpy as np
    import snesimage_amd as S
    from snesimage_amd import _ffi
    from set_characters import frames, make_set
    out = {"leg": a.leg, "frames": a.F, "version": _ffi.load().snesimage_version().decode(), "calls": a.calls, "shortlist": a.shortlist, "max_sweeps": a.sweeps}
    imgs = frames(a.F)
    if a.leg == "separate":
        st = json.load(open(a.state))
        E0, E1, tiles, sweeps = 0.0, 0.0, [], 0
        for i, img in enumerate(imgs):
            g = S.OptimizedImage(img, 8, 15)
            g.set_chunk(64)
            g.tile_palettes = np.array(st["tile_palettes"][i], np.uint8)
            g.palette = np.array(st["palette"], np.uint8)
            g.optimize()
            g.reduce_characters(st["budget"] // a.F, a.shortlist)
            e = g.error()
            E0 = e if i == 0 else E0 + e
            for _ in range(a.sweeps):
                sweeps += 1
                if g.refit_characters()[1] == 0:
                    break
            e = g.error()
            E1 = e if i == 0 else E1 + e
            tiles += json.loads(g.as_json())["tiles"]
            g.close()
        seen = set()
        for t in tiles:  # characters counted together: equal under the four flips
            c = np.array(t, np.uint8).reshape(8, 8)
            if not any(x.tobytes() in seen for x in (c, c[:, ::-1], c[::-1], c[::-1, ::-1])):
                seen.add(c.tobytes())
        out.update(error_reduced=E0, error_refitted=E1, budget=st["budget"], unique_together=len(seen), sweeps_run=sweeps)
        print(json.dumps(out))
        return 0
    ctxs, sp = make_set(S, imgs, a.calls)
    U0 = sp.characters()[0]
    budget = (U0 - a.F * a.steps) // a.F * a.F
    out.update(unique_start=U0, error_start=sp.error(), budget=budget)
    recs, U = sp.reduce_characters(budget, a.shortlist)
    out.update(merges=len(recs), unique_reduced=U, error_reduced=sp.error())
    sp.character_fits()
    t0 = time.perf_counter()
    for _ in range(3):
        reps, members, gains, fits = sp.character_fits()
    out.update(fits_ms=1e3 * (time.perf_counter() - t0) / 3, eligible=len(reps), largest_class=int(members.max()) if len(members) else 0)
    ntile = (imgs[0].shape[0] // 8) * 32
    rep = sp.characters()[1]
    out["spanning"] = sum(1 for r in reps if len({int(g) // ntile for g in np.flatnonzero(rep == r)}) > 1)
    out["sweeps"] = []
    for _ in range(a.sweeps):
        e0 = sp.error()
        t0 = time.perf_counter()
        log, acc, U, stats = sp.refit_characters()
        wall = 1e3 * (time.perf_counter() - t0)
        out["sweeps"].append(dict(wall_ms=wall, calls=len(log), accepted=acc, skipped=int((log["scored"] == 0).sum()), windows=stats["windows"], scored=stats["scored"],
                                  accepted_spanning=int(((log["changed"] == 1) & (log["touched"] > 1)).sum()), error_before=e0, error_after=sp.error(), unique=U))
        if acc == 0:
            break
    out["error_refitted"] = sp.error()
    with open(a.state, "w") as f:
        json.dump({"budget": budget, "palette": sp.palette.tolist(), "tile_palettes": [c.tile_palettes.tolist() for c in ctxs]}, f)
    sp.close()
    for c in ctxs:
        c.close()
    print(json.dumps(out))
    return 0


def run_child(a, leg, F):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--leg", leg, "--root", ROOT, "--F", str(F), "--calls", str(a.calls), "--shortlist", str(a.shortlist),
           "--steps", str(a.steps), "--sweeps", str(a.sweeps), "--state", a.state]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        print(json.dumps({"failed": cmd[2:], "rc": r.returncode, "stderr": r.stderr[-600:]}), flush=True)
        sys.exit(1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="2,4,8")
    ap.add_argument("--calls", type=int, default=240)
    ap.add_argument("--shortlist", type=int, default=16)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--sweeps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_refit_rgb.json"))
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--leg", choices=["joint", "separate"], default="joint")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--F", type=int, default=2)
    ap.add_argument("--state", default=os.path.join(ROOT, "profiles", "set_refit_state.tmp.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"runs": []}
    for F in [int(v) for v in a.frames.split(",")]:
        for leg in ("joint", "separate"):
            r = run_child(a, leg, F)
            res["runs"].append(r)
            print(json.dumps(r), flush=True)
    if os.path.exists(a.state):
        os.remove(a.state)
    res["library"] = res["runs"][0]["version"]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
