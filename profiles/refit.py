"""What the refit of shared characters (snesimage_refit_characters) gains and costs: the bench image at 256 x 224 and
256 x 256, 8 x 15, RGB, one MI355X.

    python profiles/refit.py [--calls 960] [--shortlist 16] [--sweeps 4] [--repeats R] [--baseline DIR] [--out profiles/refit_rgb.json]

The leg `refit` starts from the k-means initialisers, runs `--calls` calls of the reference's loop through snesimage_run_slots,
reduces to 512 characters (a context of its own: to 256), and then runs refit sweeps until one accepts nothing (at most
--sweeps).  It records the error before the reduction, after it and after every sweep, calls / accepted / skipped and the wall
time of every sweep (host clock around the synchronous call), and fits_ms: snesimage_character_fits at the reduced state (mean of
10 after 2) — characters, classes, the fit kernel and the copy back, an upper bound of the fit's share of a sweep.
The leg `route` is what a build without the feature has: the same state, the classes from snesimage_characters, the fit in
numpy on the host (not timed), and per class snesimage_set_palette_map + snesimage_error (and the map set back where the error
does not fall): route_ms is the wall time of those calls alone for one sweep.  --baseline DIR: a checkout of the parent commit
(its library built): `route` runs from it, the legs alternating.  Every measurement is a child process of its own under a time
limit; a child that fails ends the run: nothing more is started on the device.  The output is stamped with the library's
source hash."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGETS = (512, 256)
HEIGHTS = (224, 256)


def mean_ms(call, n=10, warm=2):
    for _ in range(warm):
        call()
    t0 = time.perf_counter()
    for _ in range(n):
        call()
    return 1e3 * (time.perf_counter() - t0) / n


def host_fits(np, g, img):
    """The eligible classes and their fits from what the parent's interface offers: [(members, flips, fitted, cur)]."""
    h = img.shape[0]
    ntile = 32 * (h // 8)

    def tiles_of(plane):
        return plane.reshape(h // 8, 8, 32, 8).transpose(0, 2, 1, 3).reshape(ntile, 64)
    _, rep, flip, _ = g.characters()
    vals = tiles_of(g.palette_map).astype(np.int64)
    orig = np.stack([tiles_of(np.ascontiguousarray(img[..., c])) for c in range(3)], axis=-1).astype(np.int64)
    pinned = (tiles_of(np.ascontiguousarray(img[..., 3])) == 0).any(axis=1)
    pal5 = g.palette.astype(np.int64)
    pal8 = ((pal5 * 8 + pal5 // 4) & 255).reshape(g.sub_count, g.sub_size, 3)
    tp = g.tile_palettes[:ntile].astype(np.int64)
    q = np.arange(64)
    out = []
    for r in np.flatnonzero(np.bincount(rep, minlength=ntile) >= 2):
        mem = np.flatnonzero(rep == r)
        if pinned[mem].any():
            continue
        cost = np.zeros((64, g.sub_size), np.int64)
        for m in mem:
            f = int(flip[m])
            a = orig[m][q ^ ((7 if f & 1 else 0) | (56 if f & 2 else 0))][:, None, :]
            b = pal8[tp[m]][None, :, :]
            rs, d = a[..., 0] + b[..., 0], a - b
            cost += (1024 + rs) * d[..., 0] ** 2 + 2048 * d[..., 1] ** 2 + (1534 - rs) * d[..., 2] ** 2
        out.append((mem, flip[mem], cost.argmin(axis=1), vals[r]))
    return out, tiles_of


def child(a):
    sys.path.insert(0, a.root)
    import numpy as np
    import snesimage_amd as S
    from snesimage_amd import _ffi
    from snesimage_amd.synth import synth_image
    img = np.ascontiguousarray(synth_image(0x5EED0000)[:a.height])
    g = S.OptimizedImage(img, 8, 15)
    g.initialize_tiles()
    g.recalculate_palettes()
    g.run_slots(a.calls, seed=1, first_step_id=0, want_log=False)
    out = {"leg": a.leg, "version": _ffi.load().snesimage_version().decode(), "calls": a.calls, "height": a.height, "budget": a.budget, "error_start": g.error(),
           "unique_start": g.characters()[0]}
    recs, unique = g.reduce_characters(a.budget, a.shortlist)
    out.update(merges=len(recs), unique=unique, error_reduced=g.error())
    if a.leg == "route":
        classes, tiles_of = host_fits(np, g, img)
        h = img.shape[0]
        inc, n_acc, n_calls, ms = g.error(), 0, 0, 0.0
        for mem, flips, fitted, cur in classes:
            if np.array_equal(fitted, cur):
                continue
            pm = g.palette_map
            vals = tiles_of(pm).copy()
            qq = np.arange(64)
            for m, f in zip(mem, flips):
                vals[m] = fitted[qq ^ ((7 if f & 1 else 0) | (56 if f & 2 else 0))]
            cand = np.ascontiguousarray(vals.reshape(h // 8, 32, 8, 8).transpose(0, 2, 1, 3).reshape(h, 256), np.uint8)
            g.sync()
            t0 = time.perf_counter()
            g.palette_map = cand
            e = g.error()
            if e < inc:
                inc, n_acc = e, n_acc + 1
            else:
                g.palette_map = pm
            ms += 1e3 * (time.perf_counter() - t0)
            n_calls += 1
        out.update(route_ms=ms, route_calls=n_calls, route_accepted=n_acc, classes=len(classes), error_route=g.error())
        print(json.dumps(out))
        return 0
    out["fits_ms"] = mean_ms(lambda: g.character_fits())
    out["sweeps"] = []
    for _ in range(a.sweeps):
        g.sync()
        t0 = time.perf_counter()
        recs, acc, unique, stats = g.refit_characters(want_stats=True)
        wall = 1e3 * (time.perf_counter() - t0)
        scored = int(recs["scored"].sum())
        out["sweeps"].append({"calls": len(recs), "accepted": acc, "skipped": len(recs) - scored, "rejected": scored - acc, "unique": unique, "error": g.error(), "wall_ms": wall,
                              "windows": stats["windows"], "scored": stats["scored"]})
        if acc == 0:
            break
    print(json.dumps(out))
    return 0


def run_child(a, root, leg, height, budget):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--leg", leg, "--root", root, "--calls", str(a.calls), "--shortlist", str(a.shortlist), "--sweeps", str(a.sweeps),
           "--height", str(height), "--budget", str(budget)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        print(json.dumps({"failed": cmd[2:], "rc": r.returncode, "stderr": r.stderr[-600:]}), flush=True)
        sys.exit(1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=960)
    ap.add_argument("--shortlist", type=int, default=16)
    ap.add_argument("--sweeps", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refit_rgb.json"))
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--leg", choices=["refit", "route"], default="refit")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--height", type=int, default=224)
    ap.add_argument("--budget", type=int, default=512)
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"runs": []}
    for _ in range(a.repeats):  # the legs alternate
        for height in HEIGHTS:
            for budget in BUDGETS:
                for leg, root in (("refit", ROOT), ("parent_route", a.baseline)):
                    if root is None:
                        continue
                    r = run_child(a, os.path.abspath(root), leg.replace("parent_", ""), height, budget)
                    r["leg"] = leg
                    res["runs"].append(r)
                    print(json.dumps(r), flush=True)
    res["library"] = next(r["version"] for r in res["runs"] if not r["leg"].startswith("parent_"))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
