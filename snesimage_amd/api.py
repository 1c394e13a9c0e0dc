"""Host-side mirror of the reference's `OptimizedImage` (src/lib.rs:33-626) over the HIP library.

Method names, argument meaning and error behaviour follow the reference: every method that the
reference declares `-> anyhow::Result<..>` raises `SnesImageError` carrying the library's message.
All arithmetic runs in libsnesimage_hip.so on the GPU; this module only marshals buffers.
"""
import ctypes as C

import numpy as np

from . import _ffi

DITHER, PERCEPTUAL, NES, BACKDROP = 1, 2, 4, 8
METHOD_RANDOM, METHOD_CHANNEL, METHOD_NES = 0, 1, 2
GUIDED_PROXIES = ("redmean", "cielab")  # SNES_GUIDE_REDMEAN, SNES_GUIDE_CIELAB
TILE_LOG_DTYPE = np.dtype([("error", np.float64), ("sub", np.int32), ("changed", np.uint8)])  # one record of a tile sweep's log
# one record of a character reduction's log (snesimage_merge_result)
MERGE_LOG_DTYPE = np.dtype([("error", np.float64), ("cost", np.uint64), ("tile", np.uint16), ("donor", np.uint16), ("flip", np.uint8), ("rank", np.uint8),
                            ("unique", np.uint16)])
# one record of a refit sweep's log (snesimage_refit_result)
REFIT_LOG_DTYPE = np.dtype([("error", np.float64), ("gain", np.uint64), ("rep", np.uint16), ("members", np.uint16), ("changed", np.uint8), ("scored", np.uint8),
                            ("pad", np.uint8, (2,))])


class SnesImageError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("snesimage_hip error %d: %s" % (code, message))
        self.code = code


def _p(a, t):
    return a.ctypes.data_as(t)


def random_candidates(seed, step_id, n):
    """Counter-RNG candidate list of (seed, step_id): n x 3 raw 5-bit (r,g,b) — lib.rs:206-208."""
    out = np.zeros((n, 3), np.uint8)
    _ffi.load().snesimage_random_candidates(seed, step_id, n, _p(out, _ffi._u8p))
    return out


def bayer_offsets(n, amplitude=32):
    """The Bayer ordered-dither table of side n (2, 4, 8 or 16) and amplitude 1..255: (n, n) int8, summing to 0
    (include/snesimage_hip.h: snesimage_bayer_offsets)."""
    n, amplitude = int(n), int(amplitude)
    if n not in (2, 4, 8, 16) or not 1 <= amplitude <= 255:
        raise ValueError("bayer_offsets: n must be 2, 4, 8 or 16 and the amplitude in 1..255")
    out = np.zeros((n, n), np.int8)
    _ffi.load().snesimage_bayer_offsets(n, amplitude, _p(out, _ffi._i8p))
    return out


def _ordered_table(table):
    """An ordered-dither table as the library takes it: contiguous (n, n) int8, or None."""
    if table is None:
        return None
    t = np.asarray(table)
    if t.ndim == 1 and t.size in (4, 16, 64, 256):
        t = t.reshape(int(round(t.size ** 0.5)), -1)
    if t.ndim != 2 or t.shape[0] != t.shape[1] or t.shape[0] not in (2, 4, 8, 16):
        raise ValueError("an ordered-dither table is (n, n) with n = 2, 4, 8 or 16")
    if t.min() < -128 or t.max() > 127:
        raise ValueError("ordered-dither offsets are int8")
    return np.ascontiguousarray(t, np.int8)


def schedule(sub_count, sub_size, n_calls, nes=False, backdrop=False):
    """Replay the slot scheduler of lib.rs:881-933: [(method, palette, index, channel, step)].
    backdrop: the schedule of a backdrop context — every sweep ends with the backdrop slot (sub_count, 0)."""
    L = _ffi.load()
    nxt = L.snesimage_schedule_next_backdrop if backdrop else L.snesimage_schedule_next
    p, i, ch, st, m = (C.c_uint32(0) for _ in range(5))
    out = []
    for _ in range(n_calls):
        cur = (p.value, i.value, ch.value, st.value)
        nxt(sub_count, sub_size, int(nes), C.byref(p), C.byref(i), C.byref(ch), C.byref(st),
                                  C.byref(m))
        out.append((m.value,) + cur)
    return out


def _native_layout(bpp, char_base, palette_base, priority):
    """snesimage_native_layout of the keyword arguments; the library judges the values, this only keeps them from wrapping."""
    bpp, char_base, palette_base, priority = int(bpp), int(char_base), int(palette_base), int(priority)
    if not (0 <= bpp <= 255 and 0 <= palette_base <= 255 and 0 <= priority <= 255 and 0 <= char_base <= 65535):
        raise ValueError("native layout: bpp, palette_base and priority are bytes, char_base a 16-bit word")
    return _ffi.NativeLayout(bpp, palette_base, priority, 0, char_base, 0)


def _export_native(owner, call, handle, ntile, frames, bpp, char_base, palette_base, priority):
    """export_native of an image (frames None) or a set (frames = F): sizes first, then the three pieces in one call."""
    layout = _native_layout(bpp, char_base, palette_base, priority)
    info = _ffi.NativeInfo()
    owner._chk(call(handle, C.byref(layout), None, None, 0, None, C.byref(info)))
    cgram, chr_ = np.zeros(512, np.uint8), np.zeros(max(int(info.chr_bytes), 1), np.uint8)
    words = np.zeros(ntile if frames is None else (frames, ntile), np.uint16)
    owner._chk(call(handle, C.byref(layout), _p(cgram, _ffi._u8p), _p(chr_, _ffi._u8p), chr_.size, _p(words, _ffi._u16p), C.byref(info)))
    return {"cgram": cgram.tobytes(), "chr": chr_[:info.chr_bytes].tobytes(), "map": words, "bpp": int(info.bpp), "unique": int(info.unique)}


def _import_native(owner, call, handle, ntile, frames, cgram, chr, map, bpp, char_base, palette_base):
    """import_native of an image (frames None) or a set (frames = F): what export_native returned, in one call."""
    cg = np.frombuffer(bytes(cgram), np.uint8) if isinstance(cgram, (bytes, bytearray, memoryview)) else np.ascontiguousarray(cgram, np.uint8).reshape(-1)
    ch = np.frombuffer(bytes(chr), np.uint8) if isinstance(chr, (bytes, bytearray, memoryview)) else np.ascontiguousarray(chr, np.uint8).reshape(-1)
    mp = np.ascontiguousarray(map, np.uint16).reshape(-1)
    if cg.size != 512 or mp.size != ntile * (1 if frames is None else frames):
        raise ValueError("import_native: cgram is 512 bytes and map holds one word per tile" + ("" if frames is None else " of every member"))
    layout = _native_layout(bpp, char_base, palette_base, 0)
    info = _ffi.NativeInfo()
    owner._chk(call(handle, C.byref(layout), _p(cg, _ffi._u8p), _p(ch, _ffi._u8p) if ch.size else None, ch.size, _p(mp, _ffi._u16p), C.byref(info)))
    return {"bpp": int(info.bpp), "unique": int(info.unique), "chr_bytes": int(info.chr_bytes), "map_words": int(info.map_words)}


class OptimizedImage:
    """`OptimizedImage::new(source, palette_count, palette_size, dither, perceptual_palettes, nes)`.

    backdrop=True (not in the reference): every tile additionally draws from one shared colour, the SNES backdrop
    (`.backdrop`).  `palette_map` then holds 0 .. sub_size, sub_size meaning backdrop, and the backdrop slot is addressed
    as (sub_count, 0) in `score_candidates`, `step` and their kin; `palette` keeps the sub_count * sub_size regular entries."""

    def __init__(self, rgba, sub_count, sub_size, dither=False, perceptual=False, nes=False, device=0, backdrop=False):
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        if rgba.ndim != 3 or rgba.shape[2] != 4:
            raise ValueError("rgba must be an (H, W, 4) uint8 array")
        self.h, self.w = int(rgba.shape[0]), int(rgba.shape[1])
        self.sub_count, self.sub_size = int(sub_count), int(sub_size)
        self.flags = (DITHER if dither else 0) | (PERCEPTUAL if perceptual else 0) | (NES if nes else 0) | (BACKDROP if backdrop else 0)
        self.has_backdrop = bool(backdrop)
        self._L = _ffi.load()
        ctx = C.c_void_p()
        rc = self._L.snesimage_create(_p(rgba, _ffi._u8p), self.w, self.h, self.sub_count, self.sub_size, self.flags,
                                      int(device), C.byref(ctx))
        if rc != 0:
            raise SnesImageError(rc, self._L.snesimage_last_error().decode())
        self._c = ctx

    # -- lifetime -------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_c", None):
            self._L.snesimage_destroy(self._c)
            self._c = None

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

    # -- plumbing -------------------------------------------------------------------------------
    def set_stream(self, hip_stream_handle):
        self._chk(self._L.snesimage_set_stream(self._c, C.c_void_p(hip_stream_handle or 0)))

    def sync(self):
        self._chk(self._L.snesimage_sync(self._c))

    def set_chunk(self, chunk):
        self._chk(self._L.snesimage_set_chunk(self._c, int(chunk)))

    def timing_enable(self, on=True):
        """True / 1: every bracket (group, H pass, V pass); 2: the V pass's only (two event records per launch group instead of six)."""
        self._chk(self._L.snesimage_timing_enable(self._c, int(on)))

    def timing_read(self):
        ms = (C.c_double * 3)()
        n, k = C.c_uint64(0), C.c_uint64(0)
        self._chk(self._L.snesimage_timing_read(self._c, ms, C.byref(n), C.byref(k)))
        return {"group_ms": ms[0], "hpass0_ms": ms[1], "vpass0_ms": ms[2], "launches": n.value, "candidates": k.value}

    # -- the reference's methods ------------------------------------------------------------------
    def initialize_tiles(self):  # lib.rs:79
        self._chk(self._L.snesimage_initialize_tiles(self._c))

    def recalculate_palettes(self):  # lib.rs:407
        self._chk(self._L.snesimage_recalculate_palettes(self._c))

    def optimize(self):  # lib.rs:425
        self._chk(self._L.snesimage_optimize(self._c))

    def error(self):  # lib.rs:503
        out = C.c_double(0)
        self._chk(self._L.snesimage_error(self._c, C.byref(out)))
        return out.value

    def reassign_tiles(self):
        """Move every tile to the subpalette that reproduces it best (not in the reference: TODO.md:36-37); tiles moved."""
        moved = C.c_uint32(0)
        self._chk(self._L.snesimage_reassign_tiles(self._c, C.byref(moved)))
        return moved.value

    def score_tile_moves(self, tiles, subs, want_maps=False):
        """error() of the image with tile tiles[j] drawn from subpalette subs[j], for every j; the state is left unchanged.
        Returns errors (float64), or (errors, maps[n, h, w]) with want_maps."""
        tiles = np.ascontiguousarray(tiles, np.uint16).reshape(-1)
        subs = np.ascontiguousarray(subs, np.uint8).reshape(-1)
        if tiles.size != subs.size:
            raise ValueError("tiles and subs differ in length")
        errs = np.zeros(tiles.size, np.float64)
        maps = np.zeros((tiles.size, self.h, self.w), np.uint8) if want_maps else None
        self._chk(self._L.snesimage_score_tile_moves(self._c, _p(tiles, _ffi._u16p), _p(subs, _ffi._u8p), tiles.size, _p(errs, _ffi._f64p),
                                                     _p(maps, _ffi._u8p) if want_maps else None))
        return (errs, maps) if want_maps else errs

    def tile_step(self, tile):
        """One tile call: the tile moves to the subpalette with the strictly lowest error(), if one beats the incumbent.
        Returns (error, sub, changed)."""
        r = _ffi.TileResult()
        self._chk(self._L.snesimage_tile_step(self._c, int(tile), C.byref(r)))
        return r.error, r.sub, int(r.changed)

    def tile_sweep(self, first_tile=0, n_tiles=None, window=0):
        """Tile calls on first_tile .. first_tile + n_tiles - 1 in order, several per launch set (bit-identical to
        `tile_step` per tile for every `window`: 0 = chosen by the library, 1 = call by call, K = at most K calls).
        Returns (log, stats): log is a structured array (error, sub, changed), one record per tile."""
        if n_tiles is None:
            n_tiles = (self.w // 8) * (self.h // 8) - int(first_tile)
        log = (_ffi.TileResult * max(1, n_tiles))()
        stats = _ffi.RunStats()
        self._chk(self._L.snesimage_tile_sweep(self._c, int(first_tile), int(n_tiles), int(window), log, C.byref(stats)))
        out = np.array([(r.error, r.sub, r.changed) for r in log[:n_tiles]], dtype=TILE_LOG_DTYPE)
        return out, {k: getattr(stats, k) for k in ("calls", "accepted", "windows", "voided", "scored", "useful")}

    # -- palette blocks (not in the reference; include/snesimage_hip.h) ----------------------------------------------
    @property
    def palette_blocks(self):
        """(bw, bh): the tiles that share one subpalette — (1, 1) per tile, (2, 2) an NES attribute area or an SNES 16 x 16 tile,
        up to (8, 8) a 64 x 64 object.  Setting it needs a tile_palettes that is constant over the new blocks (a fresh context is)."""
        bw, bh = C.c_uint32(0), C.c_uint32(0)
        self._chk(self._L.snesimage_get_palette_blocks(self._c, C.byref(bw), C.byref(bh)))
        return bw.value, bh.value

    @palette_blocks.setter
    def palette_blocks(self, v):
        bw, bh = v
        self._chk(self._L.snesimage_set_palette_blocks(self._c, int(bw), int(bh)))

    def _nblock(self):
        bw, bh = self.palette_blocks
        return (32 // bw) * ((self.h // 8) // bh)

    def score_block_moves(self, blocks, subs, want_maps=False):
        """error() of the image with every tile of block blocks[j] drawn from subpalette subs[j], for every j; the state is
        left unchanged.  Returns errors (float64), or (errors, maps[n, h, w]) with want_maps."""
        blocks = np.ascontiguousarray(blocks, np.uint16).reshape(-1)
        subs = np.ascontiguousarray(subs, np.uint8).reshape(-1)
        if blocks.size != subs.size:
            raise ValueError("blocks and subs differ in length")
        errs = np.zeros(blocks.size, np.float64)
        maps = np.zeros((blocks.size, self.h, self.w), np.uint8) if want_maps else None
        self._chk(self._L.snesimage_score_block_moves(self._c, _p(blocks, _ffi._u16p), _p(subs, _ffi._u8p), blocks.size, _p(errs, _ffi._f64p),
                                                      _p(maps, _ffi._u8p) if want_maps else None))
        return (errs, maps) if want_maps else errs

    def block_step(self, block):
        """One block call: the block moves to the subpalette with the strictly lowest error(), if one beats the incumbent.
        Returns (error, sub, changed)."""
        r = _ffi.TileResult()
        self._chk(self._L.snesimage_block_step(self._c, int(block), C.byref(r)))
        return r.error, r.sub, int(r.changed)

    def block_sweep(self, first_block=0, n_blocks=None, window=0):
        """Block calls on first_block .. first_block + n_blocks - 1 in order, several per launch set (bit-identical to
        `block_step` per block for every `window`, as `tile_sweep`).  Returns (log, stats), one record per block."""
        if n_blocks is None:
            n_blocks = self._nblock() - int(first_block)
        log = (_ffi.TileResult * max(1, n_blocks))()
        stats = _ffi.RunStats()
        self._chk(self._L.snesimage_block_sweep(self._c, int(first_block), int(n_blocks), int(window), log, C.byref(stats)))
        out = np.array([(r.error, r.sub, r.changed) for r in log[:n_blocks]], dtype=TILE_LOG_DTYPE)
        return out, {k: getattr(stats, k) for k in ("calls", "accepted", "windows", "voided", "scored", "useful")}

    # -- the character budget (not in the reference; include/snesimage_hip.h) ---------------------------------------
    def characters(self):
        """The distinct characters of the image as it stands, equal under the tilemap's flips counted once.
        Returns (unique, rep[ntile], flip[ntile], chars[ntile, 64])."""
        ntile = (self.w // 8) * (self.h // 8)
        unique = C.c_uint32(0)
        rep, flip, chars = np.zeros(ntile, np.uint16), np.zeros(ntile, np.uint8), np.zeros((ntile, 64), np.uint8)
        self._chk(self._L.snesimage_characters(self._c, C.byref(unique), _p(rep, _ffi._u16p), _p(flip, _ffi._u8p), _p(chars, _ffi._u8p)))
        return unique.value, rep, flip, chars

    def merge_shortlist(self, k=0):
        """The k (1..64, 0 = 16) merge candidates lowest in (proxy cost, tile, donor, flip); the state is left unchanged.
        Returns (tiles, donors, flips, costs), each as long as the shortlist that exists."""
        cap = 64
        tiles, donors, flips, costs = np.zeros(cap, np.uint16), np.zeros(cap, np.uint16), np.zeros(cap, np.uint8), np.zeros(cap, np.uint64)
        n = C.c_uint32(0)
        self._chk(self._L.snesimage_merge_shortlist(self._c, int(k), _p(tiles, _ffi._u16p), _p(donors, _ffi._u16p), _p(flips, _ffi._u8p), _p(costs, _ffi._u64p),
                                                    C.byref(n)))
        return tiles[:n.value].copy(), donors[:n.value].copy(), flips[:n.value].copy(), costs[:n.value].copy()

    def score_merges(self, tiles, donors, flips, want_maps=False):
        """error() of the image with tile tiles[j] taking the indices of tile donors[j] under flip flips[j], for every j; the
        state is left unchanged.  Returns errors (float64), or (errors, maps[n, h, w]) with want_maps."""
        tiles = np.ascontiguousarray(tiles, np.uint16).reshape(-1)
        donors = np.ascontiguousarray(donors, np.uint16).reshape(-1)
        flips = np.ascontiguousarray(flips, np.uint8).reshape(-1)
        if not tiles.size == donors.size == flips.size:
            raise ValueError("tiles, donors and flips differ in length")
        errs = np.zeros(tiles.size, np.float64)
        maps = np.zeros((tiles.size, self.h, self.w), np.uint8) if want_maps else None
        self._chk(self._L.snesimage_score_merges(self._c, _p(tiles, _ffi._u16p), _p(donors, _ffi._u16p), _p(flips, _ffi._u8p), tiles.size, _p(errs, _ffi._f64p),
                                                 _p(maps, _ffi._u8p) if want_maps else None))
        return (errs, maps) if want_maps else errs

    def reduce_characters(self, max_unique, shortlist=0):
        """Merge tiles until at most max_unique distinct characters are left (or no eligible pair is); every merge is the
        one of the proxy's `shortlist` (1..64, 0 = 16) best with the lowest error().  The last stage of a run: anything that
        re-runs optimize() replaces the merged map.  Returns (records, unique): a structured array (MERGE_LOG_DTYPE), one
        record per merge, and the count reached."""
        cap = (self.w // 8) * (self.h // 8)
        log = (_ffi.MergeResult * cap)()
        merges, unique = C.c_uint32(0), C.c_uint32(0)
        self._chk(self._L.snesimage_reduce_characters(self._c, int(max_unique), int(shortlist), log, cap, C.byref(merges), C.byref(unique)))
        out = np.array([(r.error, r.cost, r.tile, r.donor, r.flip, r.rank, r.unique) for r in log[:merges.value]], dtype=MERGE_LOG_DTYPE)
        return out, unique.value

    def character_fits(self):
        """The eligible classes of the image as it stands (at least two tiles sharing a character, none pinned), ascending
        representative, each with the 64 map values that cost least over all its members (include/snesimage_hip.h: FIT).
        Returns (reps[n], members[n], gains[n], fits[n, 64]); the state is left unchanged."""
        ntile = (self.w // 8) * (self.h // 8)
        reps, members, gains, fits = np.zeros(ntile, np.uint16), np.zeros(ntile, np.uint16), np.zeros(ntile, np.uint64), np.zeros((ntile, 64), np.uint8)
        n = C.c_uint32(0)
        self._chk(self._L.snesimage_character_fits(self._c, _p(reps, _ffi._u16p), _p(members, _ffi._u16p), _p(gains, _ffi._u64p), _p(fits, _ffi._u8p), C.byref(n)))
        return reps[:n.value].copy(), members[:n.value].copy(), gains[:n.value].copy(), fits[:n.value].copy()

    def score_refits(self, reps, want_maps=False):
        """error() of the image with every tile of class reps[j] redrawn from the class's fit, for every j; the state is left
        unchanged.  Returns errors (float64), or (errors, maps[n, h, w]) with want_maps."""
        reps = np.ascontiguousarray(reps, np.uint16).reshape(-1)
        errs = np.zeros(reps.size, np.float64)
        maps = np.zeros((reps.size, self.h, self.w), np.uint8) if want_maps else None
        self._chk(self._L.snesimage_score_refits(self._c, _p(reps, _ffi._u16p), reps.size, _p(errs, _ffi._f64p), _p(maps, _ffi._u8p) if want_maps else None))
        return (errs, maps) if want_maps else errs

    def refit_characters(self, window=0, want_stats=False):
        """One refit sweep: every shared character is refitted to all the tiles that use it, and the refit is kept where
        error() falls (bit-identical for every `window`: 0 = chosen by the library, 1 = call by call, K = at most K calls per
        launch set).  The last stage of a run, like `reduce_characters`.  Returns (records, accepted, unique): a structured
        array (REFIT_LOG_DTYPE), one record per eligible class, the calls taken and the character count afterwards; with
        want_stats a dict of the run statistics as a fourth item."""
        cap = (self.w // 8) * (self.h // 8)
        log = (_ffi.RefitResult * cap)()
        calls, accepted, unique = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        stats = _ffi.RunStats()
        self._chk(self._L.snesimage_refit_characters(self._c, int(window), log, cap, C.byref(calls), C.byref(accepted), C.byref(unique), C.byref(stats)))
        out = np.zeros(calls.value, REFIT_LOG_DTYPE)
        for j, r in enumerate(log[:calls.value]):
            out[j] = (r.error, r.gain, r.rep, r.members, r.changed, r.scored, (0, 0))
        if want_stats:
            return out, accepted.value, unique.value, {k: getattr(stats, k) for k in ("calls", "accepted", "windows", "voided", "scored", "useful")}
        return out, accepted.value, unique.value

    def as_tilemap_json(self):
        """The tilemap the characters imply: characters, and per tile character, hflip, vflip and palette."""
        need = self._L.snesimage_as_tilemap_json(self._c, None, 0)
        if need < 0:
            raise SnesImageError(int(need), self._L.snesimage_last_error().decode())
        buf = C.create_string_buffer(int(need))
        self._L.snesimage_as_tilemap_json(self._c, buf, need)
        return buf.value.decode()

    # -- the native export (not in the reference; include/snesimage_hip.h) ------------------------------------------
    def export_native(self, bpp=0, char_base=0, palette_base=0, priority=0):
        """The image as the console loads it (include/snesimage_hip.h, "Native export"): a dict of `cgram` (512 bytes), `chr`
        (unique * 8 * bpp bytes of bitplane characters, class order), `map` (uint16[ntile] tilemap words), `bpp` (the depth,
        resolved if 0 was given) and `unique`.  The state is left unchanged."""
        return _export_native(self, self._L.snesimage_export_native, self._c, (self.w // 8) * (self.h // 8), None, bpp, char_base, palette_base, priority)

    def render_native(self, cgram, chr, map, bpp=0, char_base=0, palette_base=0, priority=0):
        """Decode native bytes as the PPU's background fetch does -> uint8[h, w, 4], alpha 255.  Reads nothing of this
        image's palette or map: only its size, device and stream."""
        ntile = (self.w // 8) * (self.h // 8)
        cg = np.frombuffer(bytes(cgram), np.uint8)
        ch = np.frombuffer(bytes(chr), np.uint8)
        mp = np.ascontiguousarray(map, np.uint16).reshape(-1)
        if cg.size != 512 or mp.size != ntile:
            raise ValueError("render_native: cgram is 512 bytes and map holds one word per tile")
        layout = _native_layout(bpp, char_base, palette_base, priority)
        out = np.zeros((self.h, self.w, 4), np.uint8)
        self._chk(self._L.snesimage_render_native(self._c, C.byref(layout), _p(cg, _ffi._u8p), _p(ch, _ffi._u8p) if ch.size else None, ch.size, _p(mp, _ffi._u16p),
                                                  _p(out, _ffi._u8p)))
        return out

    def import_native(self, cgram, chr, map, bpp=0, char_base=0, palette_base=0):
        """Load native bytes as this image's state (include/snesimage_hip.h, "Native import"): palette, backdrop, tile_palettes
        and a stored palette_map, all or nothing.  Takes what `export_native()` returns (bytes or uint8 arrays; `map` as
        uint16[ntile]) or bytes from anywhere.  Returns a dict of `bpp`, `unique` (the cells in chr), `chr_bytes`, `map_words`."""
        return _import_native(self, self._L.snesimage_import_native, self._c, (self.w // 8) * (self.h // 8), None, cgram, chr, map, bpp, char_base, palette_base)

    def score_candidates(self, palette, index, rgb5):
        """Loop body of lib.rs:205-220 for an explicit candidate list -> errors (float64)."""
        cand = np.ascontiguousarray(rgb5, np.uint8).reshape(-1, 3)
        errs = np.zeros(cand.shape[0], np.float64)
        self._chk(self._L.snesimage_score_candidates(self._c, palette, index, _p(cand, _ffi._u8p), cand.shape[0],
                                                     _p(errs, _ffi._f64p)))
        return errs

    def score_candidates_device(self, palette, index, d_rgb5_ptr, n, d_errors_ptr, d_maps_ptr=0):
        self._chk(self._L.snesimage_score_candidates_device(self._c, palette, index, C.c_void_p(d_rgb5_ptr), n,
                                                            C.c_void_p(d_errors_ptr), C.c_void_p(d_maps_ptr or 0)))

    def remap_candidates_device(self, palette, index, d_rgb5_ptr, n, d_maps_ptr):
        """optimize() of every candidate without error(): n palette_maps into device memory (asynchronous)."""
        self._chk(self._L.snesimage_remap_candidates_device(self._c, palette, index, C.c_void_p(d_rgb5_ptr), n,
                                                            C.c_void_p(d_maps_ptr)))

    def step(self, method, palette, index, channel=0, seed=1, step_id=0, n_random=0):
        """optimize_palette_entry_{random,channel,nes} + lib.rs:906-910 -> (error, best rgb5)."""
        err = C.c_double(0)
        best = np.zeros(3, np.uint8)
        self._chk(self._L.snesimage_step(self._c, method, palette, index, channel, seed, step_id, n_random,
                                         C.byref(err), _p(best, _ffi._u8p)))
        return err.value, best

    def step_async(self, method, palette, index, channel=0, seed=1, step_id=0, n_random=0):
        self._chk(self._L.snesimage_step_async(self._c, method, palette, index, channel, seed, step_id, n_random))

    def last_step(self):
        err, k = C.c_double(0), C.c_int32(0)
        best = np.zeros(3, np.uint8)
        self._chk(self._L.snesimage_last_step(self._c, C.byref(err), _p(best, _ffi._u8p), C.byref(k)))
        return err.value, best, k.value

    def run_slots(self, n_calls, seed=1, first_step_id=0, state=(0, 0, 0, 0), window=0, want_log=True, n_random=0):
        """The reference's loop (lib.rs:888-933) for n_calls calls from scheduler state (palette, index, channel, step),
        speculatively several calls per launch (bit-identical to `step` per scheduled call).  Returns (log, state, stats):
        log[j] = (error, best_k, rgb5, changed) after call j."""
        st = [C.c_uint32(int(v)) for v in state]
        log = (_ffi.CallResult * n_calls)() if want_log else None
        stats = _ffi.RunStats()
        self._chk(self._L.snesimage_run_slots(self._c, n_calls, seed, first_step_id, C.byref(st[0]), C.byref(st[1]), C.byref(st[2]),
                                              C.byref(st[3]), int(n_random), int(window), log, C.byref(stats)))
        out = [(r.error, r.best_k, np.array(r.rgb5[:], np.uint8), int(r.changed)) for r in log] if want_log else None
        return out, tuple(v.value for v in st), {k: getattr(stats, k) for k in ("calls", "accepted", "windows", "voided", "scored", "useful")}

    def slots_reserve(self, n_slots):
        """Allocate the storage of windows of up to n_slots calls now instead of on first use."""
        self._chk(self._L.snesimage_slots_reserve(self._c, int(n_slots)))

    def slots_begin(self, n_slots, seed, first_step_id, state, n_random=0, shard_rank=0, shard_count=1, d_errors_ptr=0):
        """Phase 1 of a slot window -> (calls taken, candidates per call)."""
        taken, stride = C.c_uint32(0), C.c_uint32(0)
        self._chk(self._L.snesimage_slots_begin(self._c, n_slots, seed, first_step_id, state[0], state[1], state[2], state[3], n_random,
                                                shard_rank, shard_count, C.c_void_p(d_errors_ptr or 0), C.byref(taken), C.byref(stride)))
        return taken.value, stride.value

    def slots_commit(self, d_errors_ptr=0, n_taken=0):
        """Phase 2 -> (calls consumed, accepted flag, log of the consumed calls)."""
        used, acc = C.c_uint32(0), C.c_uint32(0)
        log = (_ffi.CallResult * max(1, n_taken))() if n_taken else None
        self._chk(self._L.snesimage_slots_commit(self._c, C.c_void_p(d_errors_ptr or 0), C.byref(used), C.byref(acc), log))
        out = [(r.error, r.best_k, np.array(r.rgb5[:], np.uint8), int(r.changed)) for r in log[:used.value]] if log else None
        return used.value, acc.value, out

    def step_begin(self, method, palette, index, channel, seed, step_id, n_total, shard_rank, shard_count,
                   d_errors_ptr):
        self._chk(self._L.snesimage_step_begin(self._c, method, palette, index, channel, seed, step_id, n_total,
                                               shard_rank, shard_count, C.c_void_p(d_errors_ptr)))

    def step_commit(self, d_errors_ptr):
        self._chk(self._L.snesimage_step_commit(self._c, C.c_void_p(d_errors_ptr)))

    # -- state ------------------------------------------------------------------------------------
    @property
    def tile_palettes(self):
        out = np.zeros(1024, np.uint8)
        self._chk(self._L.snesimage_get_tile_palettes(self._c, _p(out, _ffi._u8p)))
        return out

    @tile_palettes.setter
    def tile_palettes(self, v):
        v = np.ascontiguousarray(v, np.uint8).reshape(1024)
        self._chk(self._L.snesimage_set_tile_palettes(self._c, _p(v, _ffi._u8p)))

    @property
    def palette(self):
        out = np.zeros((self.sub_count * self.sub_size, 3), np.uint8)
        self._chk(self._L.snesimage_get_palette_rgb5(self._c, _p(out, _ffi._u8p)))
        return out

    @palette.setter
    def palette(self, v):
        v = np.ascontiguousarray(v, np.uint8).reshape(self.sub_count * self.sub_size, 3)
        self._chk(self._L.snesimage_set_palette_rgb5(self._c, _p(v, _ffi._u8p)))

    @property
    def palette_u16(self):
        out = np.zeros(self.sub_count * self.sub_size, np.uint16)
        self._chk(self._L.snesimage_get_palette_u16(self._c, _p(out, _ffi._u16p)))
        return out

    @property
    def backdrop(self):
        """The backdrop colour B, raw 5-bit (r, g, b); setting it invalidates palette_map as setting `palette` does."""
        out = np.zeros(3, np.uint8)
        self._chk(self._L.snesimage_get_backdrop_rgb5(self._c, _p(out, _ffi._u8p)))
        return out

    @backdrop.setter
    def backdrop(self, v):
        v = np.ascontiguousarray(v, np.uint8).reshape(3)
        self._chk(self._L.snesimage_set_backdrop_rgb5(self._c, _p(v, _ffi._u8p)))

    @property
    def palette_map(self):
        out = np.zeros((self.h, self.w), np.uint8)
        self._chk(self._L.snesimage_get_palette_map(self._c, _p(out, _ffi._u8p)))
        return out

    @palette_map.setter
    def palette_map(self, v):
        v = np.ascontiguousarray(v, np.uint8).reshape(self.h, self.w)
        self._chk(self._L.snesimage_set_palette_map(self._c, _p(v, _ffi._u8p)))

    def set_ordered_dither(self, table):
        """Ordered dithering (not in the reference): `table` is (n, n) int8 offsets, n = 2, 4, 8 or 16 — `bayer_offsets(n, A)`
        or any other threshold tile — added to the picture before the nearest-colour choice; None switches it off.
        Invalidates palette_map as setting `palette` does: call optimize() before reading the map or the error."""
        t = _ordered_table(table)
        if t is None:
            self._chk(self._L.snesimage_set_ordered_dither(self._c, None, 0))
        else:
            self._chk(self._L.snesimage_set_ordered_dither(self._c, _p(t, _ffi._i8p), t.shape[0]))

    @property
    def ordered_dither(self):
        """The ordered-dither table in force, (n, n) int8, or None."""
        out = np.zeros(256, np.int8)
        n = C.c_uint32(0)
        self._chk(self._L.snesimage_get_ordered_dither(self._c, _p(out, _ffi._i8p), C.byref(n)))
        return out[:n.value * n.value].reshape(n.value, n.value).copy() if n.value else None

    def set_ordered_dither_bank(self, tables, start_level=0):
        """Per-tile ordered-dither levels (not in the reference): `tables` is (L, n, n) int8, 1 <= L <= 8 tables of one side
        n = 2, 4, 8 or 16; every tile starts on `start_level`.  None switches ordered dithering off.  Invalidates
        palette_map as `set_ordered_dither` does."""
        if tables is None:
            self._chk(self._L.snesimage_set_ordered_dither_bank(self._c, None, 0, 0, 0))
            return
        t = np.asarray(tables)
        if t.ndim != 3 or t.shape[1] != t.shape[2] or t.shape[1] not in (2, 4, 8, 16):
            raise ValueError("an ordered-dither bank is (L, n, n) with n = 2, 4, 8 or 16")
        if t.min() < -128 or t.max() > 127:
            raise ValueError("ordered-dither offsets are int8")
        t = np.ascontiguousarray(t, np.int8)
        self._chk(self._L.snesimage_set_ordered_dither_bank(self._c, _p(t, _ffi._i8p), t.shape[1], t.shape[0], int(start_level)))

    @property
    def ordered_dither_bank(self):
        """The bank in force, (L, n, n) int8, or None."""
        out = np.zeros((8, 256), np.int8)
        n, L = C.c_uint32(0), C.c_uint32(0)
        self._chk(self._L.snesimage_get_ordered_dither_bank(self._c, _p(out, _ffi._i8p), C.byref(n), C.byref(L)))
        if not n.value or not L.value:
            return None
        return out[:L.value, :n.value * n.value].reshape(L.value, n.value, n.value).copy()

    @property
    def tile_levels(self):
        """The table of the bank every tile is on, 1024 uint8 as `tile_palettes`; setting it invalidates palette_map."""
        out = np.zeros(1024, np.uint8)
        self._chk(self._L.snesimage_get_tile_levels(self._c, _p(out, _ffi._u8p)))
        return out

    @tile_levels.setter
    def tile_levels(self, v):
        v = np.ascontiguousarray(v, np.uint8).reshape(1024)
        self._chk(self._L.snesimage_set_tile_levels(self._c, _p(v, _ffi._u8p)))

    def score_tile_levels(self, tiles, levels, want_maps=False):
        """error() of the image with tile tiles[j] on level levels[j], for every j; the state is left unchanged.
        Returns errors (float64), or (errors, maps[n, h, w]) with want_maps."""
        tiles = np.ascontiguousarray(tiles, np.uint16).reshape(-1)
        levels = np.ascontiguousarray(levels, np.uint8).reshape(-1)
        if tiles.size != levels.size:
            raise ValueError("tiles and levels differ in length")
        errs = np.zeros(tiles.size, np.float64)
        maps = np.zeros((tiles.size, self.h, self.w), np.uint8) if want_maps else None
        self._chk(self._L.snesimage_score_tile_levels(self._c, _p(tiles, _ffi._u16p), _p(levels, _ffi._u8p), tiles.size, _p(errs, _ffi._f64p),
                                                      _p(maps, _ffi._u8p) if want_maps else None))
        return (errs, maps) if want_maps else errs

    def level_step(self, tile):
        """One level call: the tile moves to the level with the strictly lowest error(), if one beats the incumbent.
        Returns (error, level, changed)."""
        r = _ffi.TileResult()
        self._chk(self._L.snesimage_level_step(self._c, int(tile), C.byref(r)))
        return r.error, r.sub, int(r.changed)

    def level_sweep(self, first_tile=0, n_tiles=None, window=0):
        """Level calls on first_tile .. first_tile + n_tiles - 1 in order, several per launch set (bit-identical to
        `level_step` per tile for every `window`, as `tile_sweep`).  Returns (log, stats): log is a structured array
        (error, sub, changed), `sub` holding the tile's level after the call."""
        if n_tiles is None:
            n_tiles = (self.w // 8) * (self.h // 8) - int(first_tile)
        log = (_ffi.TileResult * max(1, n_tiles))()
        stats = _ffi.RunStats()
        self._chk(self._L.snesimage_level_sweep(self._c, int(first_tile), int(n_tiles), int(window), log, C.byref(stats)))
        out = np.array([(r.error, r.sub, r.changed) for r in log[:n_tiles]], dtype=TILE_LOG_DTYPE)
        return out, {k: getattr(stats, k) for k in ("calls", "accepted", "windows", "voided", "scored", "useful")}

    # -- guided calls (not in the reference; include/snesimage_hip.h) -------------------------------------------------
    def guided_costs(self, palette, index):
        """The proxy cost of every BGR555 colour for the slot: 32,768 uint64, indexed u = r | g << 5 | b << 10 — what the
        slot's pixels would cost in the redmean key if the entry were that colour.  The state is left unchanged."""
        out = np.zeros(32768, np.uint64)
        self._chk(self._L.snesimage_guided_costs(self._c, int(palette), int(index), _p(out, _ffi._u64p)))
        return out

    def guided_candidates(self, palette, index, k=0):
        """The k (1..64, 0 = 16) colours lowest in (cost, u) but the slot's current colour, in that order; the state is
        left unchanged.  Returns (rgb5[k, 3], costs[k])."""
        n = int(k) if k else 16
        rgb5, costs = np.zeros((max(n, 1), 3), np.uint8), np.zeros(max(n, 1), np.uint64)
        self._chk(self._L.snesimage_guided_candidates(self._c, int(palette), int(index), int(k), _p(rgb5, _ffi._u8p), _p(costs, _ffi._u64p)))
        return rgb5[:n], costs[:n]

    def guided_step(self, palette, index, k=0):
        """One guided call: the shortlist of k goes through the scorer and the acceptance of `step` -> (error, best rgb5);
        `last_step` reports the record."""
        err = C.c_double(0)
        best = np.zeros(3, np.uint8)
        self._chk(self._L.snesimage_guided_step(self._c, int(palette), int(index), int(k), C.byref(err), _p(best, _ffi._u8p)))
        return err.value, best

    def guided_step_async(self, palette, index, k=0):
        self._chk(self._L.snesimage_guided_step_async(self._c, int(palette), int(index), int(k)))

    def guided_sweep(self, k=0):
        """One guided call on every slot in the schedule's order (the backdrop slot last), enqueued back to back.
        Returns (log, stats): log[j] = (error, best_k, rgb5, changed) after call j, as `run_slots` reports."""
        n = self.sub_count * self.sub_size + (1 if self.has_backdrop else 0)
        log = (_ffi.CallResult * n)()
        stats = _ffi.RunStats()
        self._chk(self._L.snesimage_guided_sweep(self._c, int(k), log, C.byref(stats)))
        out = [(r.error, r.best_k, np.array(r.rgb5[:], np.uint8), int(r.changed)) for r in log]
        return out, {k_: getattr(stats, k_) for k_ in ("calls", "accepted", "windows", "voided", "scored", "useful")}

    def guided_run_slots(self, n_calls, k=0, state=(0, 0), window=0, want_log=True):
        """n_calls guided calls of shortlist k from slot state = (palette, index) on, in the guided sweep's slot order (behind
        the last slot the first again), several calls per launch set: bit-identical to `guided_step` per call for every
        `window` (0 = adaptive, 1 = call by call).  Returns (log, state, stats) shaped like `run_slots`."""
        st = [C.c_uint32(int(v)) for v in state]
        log = (_ffi.CallResult * n_calls)() if want_log else None
        stats = _ffi.RunStats()
        self._chk(self._L.snesimage_guided_run_slots(self._c, int(n_calls), int(k), C.byref(st[0]), C.byref(st[1]), int(window), log, C.byref(stats)))
        out = [(r.error, r.best_k, np.array(r.rgb5[:], np.uint8), int(r.changed)) for r in log] if want_log else None
        return out, tuple(v.value for v in st), {k_: getattr(stats, k_) for k_ in ("calls", "accepted", "windows", "voided", "scored", "useful")}

    def debug_guided_capture(self, on=True):
        """Test hook: keep the shortlists that the calls of `guided_run_slots` score (snesimage_debug_guided_capture)."""
        self._chk(self._L.snesimage_debug_guided_capture(self._c, 1 if on else 0))

    def debug_guided_shortlists(self):
        """Test hook: the shortlists of the last captured run -> rgb5[n_calls, k, 3], in call order."""
        n, k = C.c_uint32(0), C.c_uint32(0)
        self._chk(self._L.snesimage_debug_guided_shortlists(self._c, None, 0, C.byref(n), C.byref(k)))
        out = np.zeros((n.value, k.value, 3), np.uint8)
        if out.size:
            self._chk(self._L.snesimage_debug_guided_shortlists(self._c, _p(out, _ffi._u8p), out.size, C.byref(n), C.byref(k)))
        return out

    @property
    def guided_proxy(self):
        """The metric of the guided calls' cost table: "redmean" (the default) or "cielab" — the same objective measured in
        CIEDE2000, the metric a perceptual context remaps by, in Q16 units (include/snesimage_hip.h)."""
        v = C.c_uint32(0)
        self._chk(self._L.snesimage_get_guided_proxy(self._c, C.byref(v)))
        return GUIDED_PROXIES[v.value]

    @guided_proxy.setter
    def guided_proxy(self, name):
        if name not in GUIDED_PROXIES:
            raise ValueError("guided_proxy is 'redmean' or 'cielab', not %r" % (name,))
        self._chk(self._L.snesimage_set_guided_proxy(self._c, GUIDED_PROXIES.index(name)))

    def target_rgba(self):
        """The image the nearest-colour choice is made against: the original plus the table's offsets, clamped; alpha kept."""
        out = np.zeros((self.h, self.w, 4), np.uint8)
        self._chk(self._L.snesimage_get_target_rgba(self._c, _p(out, _ffi._u8p)))
        return out

    def as_rgba(self):  # lib.rs:550
        out = np.zeros((self.h, self.w, 4), np.uint8)
        self._chk(self._L.snesimage_as_rgba(self._c, _p(out, _ffi._u8p)))
        return out

    def as_json(self):  # lib.rs:579 + .to_string() (:1002)
        need = self._L.snesimage_as_json(self._c, None, 0)
        if need < 0:
            raise SnesImageError(int(need), self._L.snesimage_last_error().decode())
        buf = C.create_string_buffer(int(need))
        self._L.snesimage_as_json(self._c, buf, need)
        return buf.value.decode()


def debug_math(op, x, y=None, device=0):
    """Evaluate the kernels' deterministic math on the GPU (bit-parity tests)."""
    L = _ffi.load()
    x = np.ascontiguousarray(x, np.float32)
    yy = x if y is None else np.ascontiguousarray(y, np.float32)
    per_in = 3 if op in (5, 6, 7, 8) else 1
    n = x.size // per_in
    out = np.zeros(n * (3 if op == 6 else 1), np.float32)
    rc = L.snesimage_debug_math(device, op, _p(x, _ffi._f32p), _p(yy, _ffi._f32p), n, _p(out, _ffi._f32p))
    if rc != 0:
        raise SnesImageError(rc, L.snesimage_last_error().decode())
    return out
