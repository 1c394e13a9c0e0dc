"""One palette shared by several images: the frames of an animated background, the poses of a sprite, the
screens of one level — on the SNES everything drawn on one background reads the same CGRAM.

`SharedPalette(images)` borrows `OptimizedImage` contexts of the same size, palette geometry, chunk and flags, all holding
the same palette, and optimizes that palette for all of them: the error of the set is the sum of the members' errors, in
member order, and every optimizer call commits once on that sum.  Each member keeps its own tile palettes and palette map.
The initialisers are the reference's own on the member stack (the members top to bottom, W x F*H).

`SharedPalette(images, backdrop=True)` (or `backdrop=(r, g, b)`) makes a backdrop set (DESIGN §5c''): every member is an
`OptimizedImage(..., backdrop=True)` and the set keeps one backdrop colour — CGRAM word 0, which all frames of a background
read — in all of them, optimized on the set's error at the backdrop slot `(sub_count, 0)`.
"""
import ctypes as C

import numpy as np

from . import _ffi
from .api import GUIDED_PROXIES, METHOD_RANDOM, TILE_LOG_DTYPE, SnesImageError, _export_native, _import_native, _p


SHARED_MERGE_LOG_DTYPE = np.dtype([("error", np.float64), ("member_error", np.float64), ("cost", np.uint64), ("member", np.uint16), ("tile", np.uint16),
                                   ("donor_member", np.uint16), ("donor", np.uint16), ("unique", np.uint16), ("flip", np.uint8), ("rank", np.uint8)])
# one record of a set's refit sweep (snesimage_shared_refit_result)
SHARED_REFIT_LOG_DTYPE = np.dtype([("error", np.float64), ("gain", np.uint64), ("rep", np.uint16), ("members", np.uint16), ("touched", np.uint16),
                                   ("changed", np.uint8), ("scored", np.uint8)])


class SharedPalette:
    """A set over `images` (OptimizedImage, in member order).  Destroy the set (close) before its members."""

    def __init__(self, images, ordered_dither=None, backdrop=None):
        """ordered_dither: an ordered-dither table (api.bayer_offsets or any (n, n) int8 tile) given to every member before the
        set is formed; None leaves the members' tables as they are (the library refuses members whose tables differ).
        backdrop: None — a plain set; True — a backdrop set (every member an OptimizedImage(..., backdrop=True)) whose B starts
        as the mean of the opaque pixels of all members; three 5-bit values — a backdrop set with that B
        (snesimage_shared_create_backdrop)."""
        self.images = list(images)
        self._L = _ffi.load()
        if ordered_dither is not None:
            for img in self.images:
                if np.ndim(ordered_dither) == 3:  # a bank, (L, n, n): with L > 1 the library refuses the member below, with its message
                    img.set_ordered_dither_bank(ordered_dither)
                else:
                    img.set_ordered_dither(ordered_dither)
        arr = (C.c_void_p * len(self.images))(*[img._c for img in self.images])
        h = C.c_void_p()
        self.has_backdrop = backdrop is not None and backdrop is not False
        if not self.has_backdrop:
            self._chk(self._L.snesimage_shared_create(arr if self.images else None, len(self.images), C.byref(h)))
        else:
            b = None if backdrop is True else np.ascontiguousarray(backdrop, np.uint8).reshape(3)
            self._chk(self._L.snesimage_shared_create_backdrop(arr if self.images else None, len(self.images), None if b is None else _p(b, _ffi._u8p), C.byref(h)))
        self._s = h
        first = self.images[0]
        self.sub_count, self.sub_size, self.flags = first.sub_count, first.sub_size, first.flags

    # -- lifetime -------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_s", None):
            self._L.snesimage_shared_destroy(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        if rc != 0:
            raise SnesImageError(rc, self._L.snesimage_last_error().decode())

    # -- the reference's methods over the set ----------------------------------------------------------
    def initialize_tiles(self):  # lib.rs:79 on the member stack
        self._chk(self._L.snesimage_shared_initialize_tiles(self._s))

    def recalculate_palettes(self):  # lib.rs:407 on the member stack
        self._chk(self._L.snesimage_shared_recalculate_palettes(self._s))

    def error(self):
        """E: the members' error() summed in member order."""
        out = C.c_double()
        self._chk(self._L.snesimage_shared_error(self._s, C.byref(out)))
        return out.value

    def score_candidates(self, palette, index, rgb5):
        """E_k for every candidate (n x 3 raw 5-bit colours) in entry (palette, index); the members are left unchanged."""
        cand = np.ascontiguousarray(rgb5, np.uint8).reshape(-1, 3)
        out = np.zeros(cand.shape[0], np.float64)
        self._chk(self._L.snesimage_shared_score_candidates(self._s, palette, index, _p(cand, _ffi._u8p), cand.shape[0],
                                                            _p(out, _ffi._f64p)))
        return out

    def step(self, method, palette, index, channel=0, seed=1, step_id=0, n_random=0):
        """One optimizer call on the set -> (E after the call, the slot's colour)."""
        err = C.c_double()
        best = np.zeros(3, np.uint8)
        self._chk(self._L.snesimage_shared_step(self._s, method, palette, index, channel, seed, step_id, n_random,
                                                C.byref(err), _p(best, _ffi._u8p)))
        return err.value, best

    def last_step(self):
        """(E, best_k, rgb5, changed) of the last call."""
        r = _ffi.CallResult()
        self._chk(self._L.snesimage_shared_last_step(self._s, C.byref(r)))
        return r.error, r.best_k, np.array(r.rgb5[:], np.uint8), int(r.changed)

    def run(self, n_calls, seed=1, first_step_id=0, state=(0, 0, 0, 0), n_random=0):
        """The reference's loop (lib.rs:888-933) on the set, call by call: n_calls calls from scheduler state
        (palette, index, channel, step), call j drawing its random candidates from (seed, first_step_id + j).
        Returns (log, state): log[j] = (E, best_k, rgb5, changed) after call j."""
        st = [C.c_uint32(int(v)) for v in state]
        m = C.c_uint32(0)
        nes = 1 if self.flags & 4 else 0
        log = []
        for j in range(n_calls):
            p, idx, ch = st[0].value, st[1].value, st[2].value
            (self._L.snesimage_schedule_next_backdrop if self.has_backdrop else self._L.snesimage_schedule_next)(self.sub_count, self.sub_size, nes, C.byref(st[0]), C.byref(st[1]), C.byref(st[2]),
                                            C.byref(st[3]), C.byref(m))
            self._chk(self._L.snesimage_shared_step_async(self._s, m.value, p, idx, ch, seed, first_step_id + j,
                                                          n_random if m.value == METHOD_RANDOM else 0))
            log.append(self.last_step())
        return log, tuple(v.value for v in st)

    def run_slots(self, n_calls, seed=1, first_step_id=0, state=(0, 0, 0, 0), window=0, want_log=True, n_random=0):
        """The same loop, several calls per launch set (snesimage_shared_run_slots): bit-identical to `run`, for every
        `window` (0 = chosen by the library, 1 = call by call, K = at most K calls per launch set).  Returns
        (log, state, stats), shaped like OptimizedImage.run_slots; log[j] = (E, best_k, rgb5, changed) after call j."""
        st = [C.c_uint32(int(v)) for v in state]
        log = (_ffi.CallResult * n_calls)() if want_log else None
        stats = _ffi.RunStats()
        self._chk(self._L.snesimage_shared_run_slots(self._s, n_calls, seed, first_step_id, C.byref(st[0]), C.byref(st[1]),
                                                     C.byref(st[2]), C.byref(st[3]), int(n_random), int(window), log, C.byref(stats)))
        out = [(r.error, r.best_k, np.array(r.rgb5[:], np.uint8), int(r.changed)) for r in log] if want_log else None
        return out, tuple(v.value for v in st), {k: getattr(stats, k) for k in ("calls", "accepted", "windows", "voided", "scored", "useful")}

    def reserve_slots(self, n):
        """Allocate the slot contexts of windows of up to n calls now instead of on first use (about 0.3 GB per member and call)."""
        self._chk(self._L.snesimage_shared_slots_reserve(self._s, int(n)))

    def reassign_tiles(self):
        """snesimage_reassign_tiles on every member -> tiles moved in all."""
        moved = C.c_uint32()
        self._chk(self._L.snesimage_shared_reassign_tiles(self._s, C.byref(moved)))
        return moved.value

    def tile_sweep(self, first_tile=0, n_tiles=None, window=0):
        """OptimizedImage.tile_sweep on every member, member after member (each call decided on the member's own error).
        Returns (log[F, n_tiles], stats)."""
        if n_tiles is None:
            n_tiles = (self.images[0].w // 8) * (self.images[0].h // 8) - int(first_tile)
        F = len(self.images)
        log = (_ffi.TileResult * max(1, F * n_tiles))()
        stats = _ffi.RunStats()
        self._chk(self._L.snesimage_shared_tile_sweep(self._s, int(first_tile), int(n_tiles), int(window), log, C.byref(stats)))
        out = np.array([(r.error, r.sub, r.changed) for r in log[:F * n_tiles]], dtype=TILE_LOG_DTYPE).reshape(F, n_tiles)
        return out, {k: getattr(stats, k) for k in ("calls", "accepted", "windows", "voided", "scored", "useful")}

    # -- guided calls of the set (not in the reference; include/snesimage_hip.h, DESIGN 5f') ---------------------------
    def guided_costs(self, palette, index):
        """The proxy cost of every BGR555 colour for the slot over all members: 32,768 uint64, indexed u = r | g << 5 | b << 10 —
        the sum of OptimizedImage.guided_costs over the members.  The state is left unchanged."""
        out = np.zeros(32768, np.uint64)
        self._chk(self._L.snesimage_shared_guided_costs(self._s, int(palette), int(index), _p(out, _ffi._u64p)))
        return out

    def guided_candidates(self, palette, index, k=0):
        """The k (1..64, 0 = 16) colours lowest in (cost, u) but the slot's current colour, in that order; the state is
        left unchanged.  Returns (rgb5[k, 3], costs[k])."""
        n = int(k) if k else 16
        rgb5, costs = np.zeros((max(n, 1), 3), np.uint8), np.zeros(max(n, 1), np.uint64)
        self._chk(self._L.snesimage_shared_guided_candidates(self._s, int(palette), int(index), int(k), _p(rgb5, _ffi._u8p), _p(costs, _ffi._u64p)))
        return rgb5[:n], costs[:n]

    def guided_step(self, palette, index, k=0):
        """One guided call on the set: every member scores the shortlist of k, the joint error decides as in `step`
        -> (E after the call, the slot's colour); `last_step` reports the record."""
        err = C.c_double(0)
        best = np.zeros(3, np.uint8)
        self._chk(self._L.snesimage_shared_guided_step(self._s, int(palette), int(index), int(k), C.byref(err), _p(best, _ffi._u8p)))
        return err.value, best

    def guided_step_async(self, palette, index, k=0):
        self._chk(self._L.snesimage_shared_guided_step_async(self._s, int(palette), int(index), int(k)))

    def guided_sweep(self, k=0):
        """One guided call on every slot in the schedule's order (the backdrop slot of a backdrop set last), enqueued back to
        back.  Returns (log, stats): log[j] = (E, best_k, rgb5, changed) after call j, as `run_slots` reports."""
        n = self.sub_count * self.sub_size + (1 if self.has_backdrop else 0)
        log = (_ffi.CallResult * n)()
        stats = _ffi.RunStats()
        self._chk(self._L.snesimage_shared_guided_sweep(self._s, int(k), log, C.byref(stats)))
        out = [(r.error, r.best_k, np.array(r.rgb5[:], np.uint8), int(r.changed)) for r in log]
        return out, {k_: getattr(stats, k_) for k_ in ("calls", "accepted", "windows", "voided", "scored", "useful")}

    def guided_run_slots(self, n_calls, k=0, state=(0, 0), window=0, want_log=True):
        """n_calls guided set calls of shortlist k from slot state = (palette, index) on, in the guided sweep's slot order (behind
        the last slot the first again), several calls per launch set (snesimage_shared_guided_run_slots): bit-identical to
        `guided_step` per call for every `window` (0 = adaptive, 1 = call by call, K = at most K calls per launch set).
        Returns (log, state, stats) shaped like `run_slots`."""
        st = [C.c_uint32(int(v)) for v in state]
        log = (_ffi.CallResult * n_calls)() if want_log else None
        stats = _ffi.RunStats()
        self._chk(self._L.snesimage_shared_guided_run_slots(self._s, int(n_calls), int(k), C.byref(st[0]), C.byref(st[1]), int(window), log, C.byref(stats)))
        out = [(r.error, r.best_k, np.array(r.rgb5[:], np.uint8), int(r.changed)) for r in log] if want_log else None
        return out, tuple(v.value for v in st), {k_: getattr(stats, k_) for k_ in ("calls", "accepted", "windows", "voided", "scored", "useful")}

    def debug_guided_capture(self, on=True):
        """Test hook: keep the shortlists that the calls of `guided_run_slots` score (snesimage_shared_debug_guided_capture)."""
        self._chk(self._L.snesimage_shared_debug_guided_capture(self._s, 1 if on else 0))

    def debug_guided_shortlists(self):
        """Test hook: the shortlists of the last captured run -> rgb5[n_calls, k, 3], in call order."""
        n, k = C.c_uint32(0), C.c_uint32(0)
        self._chk(self._L.snesimage_shared_debug_guided_shortlists(self._s, None, 0, C.byref(n), C.byref(k)))
        out = np.zeros((n.value, k.value, 3), np.uint8)
        if out.size:
            self._chk(self._L.snesimage_shared_debug_guided_shortlists(self._s, _p(out, _ffi._u8p), out.size, C.byref(n), C.byref(k)))
        return out

    def debug_guided_window_costs(self, slots):
        """Test hook: the tables of the guided windows' generator for one window whose calls are `slots`, a list of (palette,
        index), nothing scored or committed -> uint64[n, 32768], row j the final table of call j."""
        sl = np.ascontiguousarray(slots, np.uint32).reshape(-1, 2)
        p, i = np.ascontiguousarray(sl[:, 0]), np.ascontiguousarray(sl[:, 1])
        out = np.zeros((max(len(sl), 1), 32768), np.uint64)
        self._chk(self._L.snesimage_shared_debug_guided_window_costs(self._s, _p(p, _ffi._u32p), _p(i, _ffi._u32p), len(sl), _p(out, _ffi._u64p)))
        return out[:len(sl)]

    @property
    def guided_proxy(self):
        """The metric of the set's guided cost table: "redmean" (the default) or "cielab".  The set's own setting: the
        members' `guided_proxy` is neither read nor written."""
        v = C.c_uint32(0)
        self._chk(self._L.snesimage_shared_get_guided_proxy(self._s, C.byref(v)))
        return GUIDED_PROXIES[v.value]

    @guided_proxy.setter
    def guided_proxy(self, name):
        if name not in GUIDED_PROXIES:
            raise ValueError("guided_proxy is 'redmean' or 'cielab', not %r" % (name,))
        self._chk(self._L.snesimage_shared_set_guided_proxy(self._s, GUIDED_PROXIES.index(name)))

    # -- per-tile ordered-dither levels of the set, tied or per frame (not in the reference; include/snesimage_hip.h) ----
    def set_ordered_dither_bank(self, bank, start_level=0):
        """The set's bank: `bank` is (L, n, n) int8, 1 <= L <= 8 tables of one side n = 2, 4, 8 or 16, given to every member
        with every tile of every member on `start_level`; None switches the tables of all members off.  The set is settled
        afterwards (optimize() has run on every member)."""
        if bank is None:
            self._chk(self._L.snesimage_shared_set_ordered_dither_bank(self._s, None, 0, 0, 0))
            return
        t = np.asarray(bank)
        if t.ndim != 3 or t.shape[1] != t.shape[2] or t.shape[1] not in (2, 4, 8, 16):
            raise ValueError("an ordered-dither bank is (L, n, n) with n = 2, 4, 8 or 16")
        if t.min() < -128 or t.max() > 127:
            raise ValueError("ordered-dither offsets are int8")
        t = np.ascontiguousarray(t, np.int8)
        self._chk(self._L.snesimage_shared_set_ordered_dither_bank(self._s, _p(t, _ffi._i8p), t.shape[1], t.shape[0], int(start_level)))

    def set_tile_levels(self, member, levels):
        """OptimizedImage.tile_levels = levels on member `member` of the set (1024 uint8); the set is settled afterwards."""
        v = np.ascontiguousarray(levels, np.uint8).reshape(1024)
        self._chk(self._L.snesimage_shared_set_tile_levels(self._s, int(member), _p(v, _ffi._u8p)))

    @property
    def tile_levels(self):
        """The level every tile of every member is on, (F, 1024) uint8."""
        return np.stack([img.tile_levels for img in self.images])

    def score_tile_levels(self, tiles, levels):
        """E of the set with EVERY member's tile tiles[j] on level levels[j], for every j; the state is left unchanged.
        Returns (errors[n], member_errors[n, F]): a member already on that level keeps its incumbent bit for bit."""
        tiles = np.ascontiguousarray(tiles, np.uint16).reshape(-1)
        levels = np.ascontiguousarray(levels, np.uint8).reshape(-1)
        if tiles.size != levels.size:
            raise ValueError("tiles and levels differ in length")
        errs, mem = np.zeros(tiles.size, np.float64), np.zeros((tiles.size, len(self.images)), np.float64)
        self._chk(self._L.snesimage_shared_score_tile_levels(self._s, _p(tiles, _ffi._u16p), _p(levels, _ffi._u8p), tiles.size, _p(errs, _ffi._f64p), _p(mem, _ffi._f64p)))
        return errs, mem

    def level_sweep(self, first_tile=0, n_tiles=None, window=0, tied=True):
        """tied: tied level calls on tile positions first_tile .. first_tile + n_tiles - 1 in order — one level per position for
        all members, decided on E (a single member's error may rise) — several per launch set, bit-identical for every `window`
        (0 = chosen by the library, 1 = call by call, K = at most K calls per launch set); log[n_tiles] holds (E, the common
        level, changed).  Not tied: OptimizedImage.level_sweep on every member, member after member, each call decided on the
        member's own error; log[F, n_tiles].  Returns (log, stats)."""
        if n_tiles is None:
            n_tiles = self._ntile() - int(first_tile)
        F = 1 if tied else len(self.images)
        log = (_ffi.TileResult * max(1, F * n_tiles))()
        stats = _ffi.RunStats()
        self._chk(self._L.snesimage_shared_level_sweep(self._s, int(first_tile), int(n_tiles), int(window), 1 if tied else 0, log, C.byref(stats)))
        out = np.array([(r.error, r.sub, r.changed) for r in log[:F * n_tiles]], dtype=TILE_LOG_DTYPE)
        if not tied:
            out = out.reshape(F, n_tiles)
        return out, {k: getattr(stats, k) for k in ("calls", "accepted", "windows", "voided", "scored", "useful")}

    # -- the character budget of the set (not in the reference; include/snesimage_hip.h) ---------------------------
    def _ntile(self):
        return (self.images[0].w // 8) * (self.images[0].h // 8)

    def characters(self):
        """The distinct characters of all members together (global tile g = member * ntile + tile), equal under the tilemap's
        flips counted once.  Returns (unique, rep[G] as global indices, flip[G], chars[G, 64])."""
        G = len(self.images) * self._ntile()
        unique = C.c_uint32(0)
        rep, flip, chars = np.zeros(G, np.uint16), np.zeros(G, np.uint8), np.zeros((G, 64), np.uint8)
        self._chk(self._L.snesimage_shared_characters(self._s, C.byref(unique), _p(rep, _ffi._u16p), _p(flip, _ffi._u8p), _p(chars, _ffi._u8p)))
        return unique.value, rep, flip, chars

    def merge_shortlist(self, k=0):
        """The k (1..64, 0 = 16) merge candidates lowest in (proxy cost, recipient, donor, flip) over the whole set; the state
        is left unchanged.  Returns (members, tiles, donor_members, donors, flips, costs), each as long as the shortlist."""
        cap = 64
        mem, tiles, dmem, donors = (np.zeros(cap, np.uint16) for _ in range(4))
        flips, costs = np.zeros(cap, np.uint8), np.zeros(cap, np.uint64)
        n = C.c_uint32(0)
        self._chk(self._L.snesimage_shared_merge_shortlist(self._s, int(k), _p(mem, _ffi._u16p), _p(tiles, _ffi._u16p), _p(dmem, _ffi._u16p), _p(donors, _ffi._u16p),
                                                           _p(flips, _ffi._u8p), _p(costs, _ffi._u64p), C.byref(n)))
        return tuple(a[:n.value].copy() for a in (mem, tiles, dmem, donors, flips, costs))

    def score_merges(self, members, tiles, donor_members, donors, flips, want_maps=False):
        """error() of member members[j] with its tile tiles[j] taking the indices of tile donors[j] of member donor_members[j]
        under flip flips[j], for every j; the state is left unchanged.  Returns errors (float64), or (errors, maps[n, h, w])."""
        mem, tiles, dmem, donors = (np.ascontiguousarray(a, np.uint16).reshape(-1) for a in (members, tiles, donor_members, donors))
        flips = np.ascontiguousarray(flips, np.uint8).reshape(-1)
        if not mem.size == tiles.size == dmem.size == donors.size == flips.size:
            raise ValueError("members, tiles, donor_members, donors and flips differ in length")
        errs = np.zeros(mem.size, np.float64)
        maps = np.zeros((mem.size, self.images[0].h, self.images[0].w), np.uint8) if want_maps else None
        self._chk(self._L.snesimage_shared_score_merges(self._s, _p(mem, _ffi._u16p), _p(tiles, _ffi._u16p), _p(dmem, _ffi._u16p), _p(donors, _ffi._u16p),
                                                        _p(flips, _ffi._u8p), mem.size, _p(errs, _ffi._f64p), _p(maps, _ffi._u8p) if want_maps else None))
        return (errs, maps) if want_maps else errs

    def reduce_characters(self, max_unique, shortlist=0):
        """Merge tiles until the whole set holds at most max_unique distinct characters (or no eligible pair is left); a donor
        may sit in another member.  Every merge is the one of the proxy's `shortlist` (1..64, 0 = 16) best that raises its
        member's error() least.  The last stage of a run: any set call that optimizes replaces the merged maps.  Returns
        (records, unique): a structured array (SHARED_MERGE_LOG_DTYPE), one record per merge, and the count reached."""
        cap = len(self.images) * self._ntile()
        log = (_ffi.SharedMergeResult * cap)()
        merges, unique = C.c_uint32(0), C.c_uint32(0)
        self._chk(self._L.snesimage_shared_reduce_characters(self._s, int(max_unique), int(shortlist), log, cap, C.byref(merges), C.byref(unique)))
        out = np.array([(r.error, r.member_error, r.cost, r.member, r.tile, r.donor_member, r.donor, r.unique, r.flip, r.rank) for r in log[:merges.value]],
                       dtype=SHARED_MERGE_LOG_DTYPE)
        return out, unique.value

    def character_fits(self):
        """The eligible classes of the set as it stands (at least two tiles, of whichever members, sharing a character, none
        pinned), ascending global representative, each with the 64 map values that cost least over all its tiles
        (include/snesimage_hip.h: FIT).  Returns (reps[n], members[n], gains[n], fits[n, 64]); the state is left unchanged."""
        G = len(self.images) * self._ntile()
        reps, members, gains, fits = np.zeros(G, np.uint16), np.zeros(G, np.uint16), np.zeros(G, np.uint64), np.zeros((G, 64), np.uint8)
        n = C.c_uint32(0)
        self._chk(self._L.snesimage_shared_character_fits(self._s, _p(reps, _ffi._u16p), _p(members, _ffi._u16p), _p(gains, _ffi._u64p), _p(fits, _ffi._u8p), C.byref(n)))
        return reps[:n.value].copy(), members[:n.value].copy(), gains[:n.value].copy(), fits[:n.value].copy()

    def score_refits(self, reps, maps=False):
        """E' of the set with every tile of class reps[j] (a global representative) redrawn from the class's fit, for every j;
        the state is left unchanged.  Returns (errors[n], member_errors[n, F]) — a member the class does not touch keeps its
        incumbent — and with maps=True also maps[n, F, h, w]."""
        reps = np.ascontiguousarray(reps, np.uint16).reshape(-1)
        F = len(self.images)
        errs, mem = np.zeros(reps.size, np.float64), np.zeros((reps.size, F), np.float64)
        out = np.zeros((reps.size, F, self.images[0].h, self.images[0].w), np.uint8) if maps else None
        self._chk(self._L.snesimage_shared_score_refits(self._s, _p(reps, _ffi._u16p), reps.size, _p(errs, _ffi._f64p), _p(mem, _ffi._f64p), _p(out, _ffi._u8p) if maps else None))
        return (errs, mem, out) if maps else (errs, mem)

    def refit_characters(self, window=0, log_cap=None):
        """One refit sweep over the set: every character shared by tiles of whichever members is refitted to all of them, and
        the refit is kept where E falls (a single member's error may rise).  Bit-identical for every `window` (0 = chosen by the
        library, 1 = call by call, K = at most K calls per launch set).  The last stage of a run, like `reduce_characters`.
        Returns (records, accepted, unique, stats): a structured array (SHARED_REFIT_LOG_DTYPE) of the first log_cap records
        (default: all), one per eligible class, the calls taken, the character count afterwards and the run statistics."""
        cap = len(self.images) * self._ntile() if log_cap is None else int(log_cap)
        log = (_ffi.SharedRefitResult * max(1, cap))()
        calls, accepted, unique = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        stats = _ffi.RunStats()
        self._chk(self._L.snesimage_shared_refit_characters(self._s, int(window), log, cap, C.byref(calls), C.byref(accepted), C.byref(unique), C.byref(stats)))
        n = min(calls.value, cap)
        out = np.zeros(n, SHARED_REFIT_LOG_DTYPE)
        for j, r in enumerate(log[:n]):
            out[j] = (r.error, r.gain, r.rep, r.members, r.touched, r.changed, r.scored)
        return out, accepted.value, unique.value, {k: getattr(stats, k) for k in ("calls", "accepted", "windows", "voided", "scored", "useful")}

    def as_tilemap_json(self):
        """The tilemap of the set: one list of characters, and per member and tile character, hflip, vflip and palette."""
        need = self._L.snesimage_shared_as_tilemap_json(self._s, None, 0)
        if need < 0:
            raise SnesImageError(int(need), self._L.snesimage_last_error().decode())
        buf = C.create_string_buffer(int(need))
        self._L.snesimage_shared_as_tilemap_json(self._s, buf, need)
        return buf.value.decode()

    def export_native(self, bpp=0, char_base=0, palette_base=0, priority=0):
        """The set as the console loads it (include/snesimage_hip.h, "Native export"): as OptimizedImage.export_native, with
        ONE `chr` for all members (classes counted over the whole set) and `map` of shape [F, ntile], member order."""
        return _export_native(self, self._L.snesimage_shared_export_native, self._s, self._ntile(), len(self.images), bpp, char_base, palette_base, priority)

    def import_native(self, cgram, chr, maps, bpp=0, char_base=0, palette_base=0):
        """Load native bytes as the state of the set (include/snesimage_hip.h, "Native import"): one palette for all members,
        each member's tile_palettes and stored map from its row of `maps` ([F, ntile]); all or nothing over the whole set."""
        return _import_native(self, self._L.snesimage_shared_import_native, self._s, self._ntile(), len(self.images), cgram, chr, maps, bpp, char_base, palette_base)

    # -- state ------------------------------------------------------------------------------------
    @property
    def palette(self):
        """The shared palette: sub_count * sub_size entries (on a backdrop set the regular entries; B is `backdrop`)."""
        return self.images[0].palette

    @property
    def backdrop(self):
        """B of a backdrop set (three raw 5-bit values); setting it writes all tied entries of all members, then optimize()."""
        out = np.zeros(3, np.uint8)
        self._chk(self._L.snesimage_shared_get_backdrop_rgb5(self._s, _p(out, _ffi._u8p)))
        return out

    @backdrop.setter
    def backdrop(self, v):
        v = np.ascontiguousarray(v, np.uint8).reshape(3)
        self._chk(self._L.snesimage_shared_set_backdrop_rgb5(self._s, _p(v, _ffi._u8p)))

    @palette.setter
    def palette(self, v):
        v = np.ascontiguousarray(v, np.uint8).reshape(self.sub_count * self.sub_size, 3)
        self._chk(self._L.snesimage_shared_set_palette_rgb5(self._s, _p(v, _ffi._u8p)))
