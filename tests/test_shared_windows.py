"""Slot windows for a set (snesimage_shared_run_slots, SharedPalette.run_slots, cli --share with --window 0): several calls
of the reference's loop per launch set on one palette shared by F frames.  The contract is one sentence — for every window
size, everything observable afterwards equals snesimage_schedule_next + snesimage_shared_step per call, bit for bit — so
the yardstick is the product's own call-by-call loop (SharedPalette.run), which tests/test_shared_palette.py holds against
the oracle; one test here goes to the oracle directly."""
import ctypes as C
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")
REL = 1e-11  # tests/test_shared_palette.py's bound against the oracle
WINDOW_FUNCS = ["snesimage_shared_run_slots", "snesimage_shared_slots_reserve"]


def rel(a, b):
    return abs(a - b) / abs(b)


def write_png(path, rgba):
    h, w = rgba.shape[:2]
    raw = b"".join(b"\x00" + rgba[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    path.write_bytes(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) +
                     chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


# ---- without a device ------------------------------------------------------------------------------------------------------

def test_window_symbols_exported_declared_and_bound():
    from snesimage_amd import _ffi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snesimage_hip.h")).read(), flags=re.S)
    lib = _ffi.load()
    bound = {n for n, _, _ in _ffi.SIGNATURES}
    for name in WINDOW_FUNCS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in bound and getattr(lib, name) is not None
    st = [C.c_uint32(0) for _ in range(4)]
    assert lib.snesimage_shared_run_slots(None, 1, 1, 0, *[C.byref(v) for v in st], 0, 0, None, None) == -1
    assert lib.snesimage_shared_slots_reserve(None, 4) == -1
    from snesimage_amd.shared import SharedPalette
    assert callable(SharedPalette.run_slots) and callable(SharedPalette.reserve_slots)


# ---- on the MI355X ---------------------------------------------------------------------------------------------------------

def frames(F, H, variant=0, seed=0x5EED7000):
    from snesimage_amd.synth import synth_image
    return [synth_image(seed + i, 256, H, variant) for i in range(F)]


def make_set(imgs, sub_count, sub_size, **flags):
    """A set at the k-means initialisers (deterministic: two sets from the same frames are in the same state)."""
    import snesimage_amd as S
    ctxs = [S.OptimizedImage(f, sub_count, sub_size, device=0, **flags) for f in imgs]
    for c in ctxs:
        c.set_chunk(64)
    sp = S.SharedPalette(ctxs)
    sp.initialize_tiles()
    sp.recalculate_palettes()
    return ctxs, sp


def close(ctxs, sp):
    sp.close()
    for c in ctxs:
        c.close()


def state_at(sub_count, sub_size, call, nes=False):
    import snesimage_amd as S
    _, p, i, ch, st = S.schedule(sub_count, sub_size, call + 1, nes)[call]
    return (p, i, ch, st)


def bits(log):
    """Every record as bytes: the error's 8 bytes, best_k, rgb5, changed."""
    return [(struct.pack("<d", e), int(k), bytes(bytearray(c.tolist())), int(ch)) for e, k, c, ch in log]


def snapshot(ctxs, sp):
    """Everything a caller can see of the set and its members, errors as their 8 bytes."""
    e, k, c, ch = sp.last_step()
    out = [("joint", struct.pack("<d", e), k, c.tolist(), ch)]
    for m in ctxs:
        le, lb, lk = m.last_step()
        out.append((m.palette.tobytes(), m.palette_map.tobytes(), m.tile_palettes.tobytes(), struct.pack("<d", m.error()),
                    struct.pack("<d", le), lb.tolist(), lk))
    return out


CASES = {
    "rgb": dict(F=3, H=80, count=2, size=3, flags={}, first=0, n=60),
    "perceptual": dict(F=3, H=80, count=2, size=3, flags={"perceptual": True}, first=0, n=60),
    "dither": dict(F=3, H=80, count=2, size=3, flags={"dither": True}, first=0, n=60),
    "nes": dict(F=2, H=80, count=2, size=3, flags={"nes": True}, first=0, n=60),
    # the real geometry; calls 440..479 are random calls of step 3, 480.. the channel sweep of step 4
    "256x224_8x15": dict(F=4, H=224, count=8, size=15, flags={}, first=440, n=100),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_windows_equal_call_by_call(name):
    import snesimage_amd as S
    c = CASES[name]
    nes = bool(c["flags"].get("nes"))
    imgs = frames(c["F"], c["H"], 1 if name != "256x224_8x15" else 0)
    sched = S.schedule(c["count"], c["size"], c["first"] + c["n"], nes)[c["first"]:]
    methods = {m for m, *_ in sched}
    assert methods == ({S.METHOD_NES} if nes else {S.METHOD_RANDOM, S.METHOD_CHANNEL})  # the run crosses into a channel sweep
    start, end = state_at(c["count"], c["size"], c["first"], nes), state_at(c["count"], c["size"], c["first"] + c["n"], nes)
    rc, rs = make_set(imgs, c["count"], c["size"], **c["flags"])
    want, st = rs.run(c["n"], seed=7, first_step_id=c["first"], state=start)
    assert st == end
    assert sum(ch for *_, ch in want) >= 3  # from the k-means start: the windows are cut by acceptances
    want_snap = snapshot(rc, rs)
    for window in (0, 2, 5, 16):
        gc, gs = make_set(imgs, c["count"], c["size"], **c["flags"])
        got, st, stats = gs.run_slots(c["n"], seed=7, first_step_id=c["first"], state=start, window=window)
        assert st == end, window
        assert bits(got) == bits(want), window
        assert snapshot(gc, gs) == want_snap, window
        assert stats["calls"] == c["n"] and stats["scored"] >= stats["useful"]
        assert stats["accepted"] == sum((ch if nes else k >= 0) for _, k, _, ch in want)
        if window != 0:
            assert stats["windows"] < c["n"], (window, stats)  # several calls per launch set did happen
        close(gc, gs)
    close(rc, rs)


@pytest.mark.gpu
def test_a_run_in_pieces_and_across_reassign_tiles():
    """first_step_id and the scheduler state handed on from piece to piece; reassign_tiles() between two pieces; a
    call-by-call piece between two windowed ones."""
    imgs = frames(3, 80, 1, seed=0x5EED7100)
    rc, rs = make_set(imgs, 2, 3)
    gc, gs = make_set(imgs, 2, 3)
    want, st_w = rs.run(25, seed=4)
    more, st_w = rs.run(35, seed=4, first_step_id=25, state=st_w)
    want += more
    got, st_g, done = [], (0, 0, 0, 0), 0
    for piece, window in ((9, 4), (1, 0), (15, 1), (35, 0)):
        l, st_g, _ = gs.run_slots(piece, seed=4, first_step_id=done, state=st_g, window=window)
        got += l
        done += piece
    assert st_g == st_w and bits(got) == bits(want)
    assert snapshot(gc, gs) == snapshot(rc, rs)
    assert rs.reassign_tiles() == gs.reassign_tiles()
    want, st_w = rs.run(30, seed=4, first_step_id=60, state=st_w)
    got, st_g, _ = gs.run_slots(30, seed=4, first_step_id=60, state=st_g, window=6)
    assert st_g == st_w and bits(got) == bits(want)
    assert snapshot(gc, gs) == snapshot(rc, rs)
    # a set call of another kind goes on from there
    import snesimage_amd as S
    assert struct.pack("<d", rs.step(S.METHOD_RANDOM, 0, 1, 0, 4, 90, 16)[0]) == struct.pack("<d", gs.step(S.METHOD_RANDOM, 0, 1, 0, 4, 90, 16)[0])
    assert struct.pack("<d", rs.error()) == struct.pack("<d", gs.error())
    close(rc, rs)
    close(gc, gs)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [{}, {"dither": True}])
def test_windowed_trajectory_follows_the_summed_oracle(O, flags):
    """tests/test_shared_palette.py's model — the members' oracle scores summed in member order, the reference's rule on
    the sum — for 24 calls with 16 random candidates through run_slots(window=8)."""
    imgs = frames(3, 80, 1, seed=0x5EED5200)
    ctxs, sp = make_set(imgs, 2, 3, **flags)
    oms = []
    for f, c in zip(imgs, ctxs):
        o = O.OracleImage(f, 2, 3, **flags)
        o.tile_palettes = c.tile_palettes
        o.palette = c.palette
        o.optimize()
        oms.append(o)
    pal = oms[0].palette
    seed, n_random = 9, 16
    log, _, stats = sp.run_slots(24, seed=seed, first_step_id=0, window=8, n_random=n_random)
    assert stats["calls"] == 24
    for j, (method, p, idx, ch, _) in enumerate(O.schedule(2, 3, 24)):
        assert method == 0
        cand = O.random_candidates(seed, j, n_random)
        inc = 0.0
        for o in oms:
            inc = inc + o.error()
        E = None
        for o in oms:
            e = o.score_candidates(p, idx, cand)
            E = e if E is None else E + e
        k = int(np.argmin(E))  # the first index of the minimum
        slot = p * 3 + idx
        if E[k] < inc:
            pal[slot] = cand[k]
            for o in oms:
                o.palette = pal
                o.optimize()
        e_g, k_g, rgb_g, _ = log[j]
        assert np.array_equal(rgb_g, pal[slot]), j
        assert (k_g == k) == bool(E[k] < inc), j
        assert rel(e_g, E[k] if E[k] < inc else inc) < REL, j
    for c, o in zip(ctxs, oms):
        assert np.array_equal(c.palette, pal) and np.array_equal(c.palette_map, o.palette_map)
    close(ctxs, sp)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [{}, {"dither": True}])
def test_a_set_of_one_runs_as_a_plain_context(flags):
    import snesimage_amd as S
    from snesimage_amd.synth import synth_image
    img = synth_image(0x5EED7300, 256, 64, 1)
    solo = S.OptimizedImage(img, 2, 3, device=0, **flags)
    solo.set_chunk(64)
    solo.initialize_tiles()
    solo.recalculate_palettes()
    ctxs, sp = make_set([img], 2, 3, **flags)
    assert np.array_equal(solo.palette, ctxs[0].palette) and np.array_equal(solo.tile_palettes, ctxs[0].tile_palettes)
    want, st_w, _ = solo.run_slots(60, seed=5, window=7)
    got, st_g, _ = sp.run_slots(60, seed=5, window=7)
    assert st_g == st_w and bits(got) == bits(want)
    assert np.array_equal(ctxs[0].palette, solo.palette) and np.array_equal(ctxs[0].palette_map, solo.palette_map)
    assert struct.pack("<d", ctxs[0].error()) == struct.pack("<d", solo.error())
    close(ctxs, sp)
    solo.close()


@pytest.mark.gpu
@pytest.mark.parametrize("F,K", [(3, 5), (2, 16), (4, 16)])
def test_stats_and_the_bound_on_launch_sets(F, K):
    """Every launch set ends on an acceptance, on a method change, or holds K calls (F * K <= 64, the default storage cap);
    the last one may be short: windows <= accepted + ceil(n / K) + (method changes + 1)."""
    import snesimage_amd as S
    n = 60
    imgs = frames(F, 80, 0, seed=0x5EED7400)
    ctxs, sp = make_set(imgs, 2, 3)
    sched = S.schedule(2, 3, n)
    per_call = [64 if m == S.METHOD_RANDOM else 32 for m, *_ in sched]
    changes = sum(1 for a, b in zip(sched, sched[1:]) if a[0] != b[0])
    log, _, stats = sp.run_slots(n, seed=11, window=K)
    assert stats["calls"] == n
    assert stats["accepted"] == sum(k >= 0 for _, k, _, _ in log)
    assert stats["useful"] == sum(per_call)
    assert stats["scored"] >= stats["useful"]
    assert stats["windows"] <= stats["accepted"] + -(-n // K) + changes + 1, stats
    close(ctxs, sp)


@pytest.mark.gpu
def test_state_and_lifetime():
    import snesimage_amd as S
    from snesimage_amd import _ffi
    L = _ffi.load()
    imgs = frames(2, 64, 0, seed=0x5EED7500)
    # a failed reserve (SNES_ERR_HIP) leaves the set usable: its windows still equal call by call
    rc, rs = make_set(imgs, 2, 3)
    gc, gs = make_set(imgs, 2, 3)
    failures = 0
    for nth in (0, 1, 3, 6, 10, 15, 21, 28, 36, 60, 100):
        L.snesimage_debug_fail_alloc(nth)
        try:
            gs.reserve_slots(6)
            ok = True
        except S.SnesImageError as e:
            assert e.code == -2
            ok = False
            failures += 1
        finally:
            L.snesimage_debug_fail_alloc(-1)
        if ok:
            break
    assert failures >= 3
    want, st_w = rs.run(40, seed=6)
    got, st_g, stats = gs.run_slots(40, seed=6, window=6)
    assert st_g == st_w and bits(got) == bits(want) and snapshot(gc, gs) == snapshot(rc, rs)
    assert stats["windows"] < 40
    close(rc, rs)
    # a member changed through its own call: SNES_ERR_STATE
    pal = gc[1].palette
    pal[1] = (pal[1] + 3) % 32
    gc[1].palette = pal
    with pytest.raises(S.SnesImageError) as e:
        gs.run_slots(4, seed=6, first_step_id=40, state=st_g)
    assert e.value.code == -3
    with pytest.raises(S.SnesImageError) as e:
        gs.reserve_slots(2)
    assert e.value.code == -3
    close(gc, gs)
    # a retired set
    ctxs, sp = make_set(imgs, 2, 3)
    sp.run_slots(8, seed=6, window=4)
    ctxs[1].close()
    with pytest.raises(S.SnesImageError) as e:
        sp.run_slots(4, seed=6)
    assert e.value.code == -3
    sp.close()
    ctxs[0].close()


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--reassign-tiles", "1"]], ids=["plain", "reassign"])
def test_cli_share_windows_write_the_same_files(tmp_path, extra):
    """--share for two extra frames, 120 calls: the three JSON files are byte-identical between --window 0 and --window 1."""
    imgs = frames(3, 64, 1, seed=0x5EED7600)
    for i, f in enumerate(imgs):
        write_png(tmp_path / ("f%d.png" % i), f)
    outs = {}
    for window in ("0", "1"):
        names = [str(tmp_path / ("w%s_o%d.json" % (window, i))) for i in range(3)]
        r = subprocess.run([CLI, str(tmp_path / "f0.png"), names[0], "--share", "%s=%s" % (tmp_path / "f1.png", names[1]),
                            "--share", "%s=%s" % (tmp_path / "f2.png", names[2]), "-c", "2", "-s", "3", "--calls", "120",
                            "--window", window, *extra], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "Current Error" in r.stdout and "Sharing one palette between 3 images" in r.stdout
        if window == "0":
            assert "launch sets" in r.stdout
        outs[window] = [open(n, "rb").read() for n in names]
        errors = re.findall(r"Current Error: (\S+)", r.stdout)
        outs[window].append(errors)
    assert outs["0"][:3] == outs["1"][:3]
    assert outs["0"][3] == outs["1"][3]  # the same E after every call that moved it
