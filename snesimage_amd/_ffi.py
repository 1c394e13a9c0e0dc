"""ctypes binding of libsnesimage_hip.so (the C ABI declared in include/snesimage_hip.h).

The library is built in-tree by `make -C snesimage_amd/csrc` (or __graft_entry__.build()).
There is no fallback: if the shared object is missing, importing the binding raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libsnesimage_hip.so")

_u8p = C.POINTER(C.c_uint8)
_i8p = C.POINTER(C.c_int8)
_u16p = C.POINTER(C.c_uint16)
_u32p = C.POINTER(C.c_uint32)
_i32p = C.POINTER(C.c_int32)
_u64p = C.POINTER(C.c_uint64)
_f32p = C.POINTER(C.c_float)
_f64p = C.POINTER(C.c_double)



class CallResult(C.Structure):
    """snesimage_call_result: what snesimage_last_step reports after one optimizer call."""
    _fields_ = [("error", C.c_double), ("best_k", C.c_int32), ("rgb5", C.c_uint8 * 3), ("changed", C.c_uint8)]


class RunStats(C.Structure):
    """snesimage_run_stats"""
    _fields_ = [("calls", C.c_uint32), ("accepted", C.c_uint32), ("windows", C.c_uint32), ("voided", C.c_uint32),
                ("scored", C.c_uint64), ("useful", C.c_uint64)]


class TileResult(C.Structure):
    """snesimage_tile_result: incumbent error and the tile's subpalette after a tile call."""
    _fields_ = [("error", C.c_double), ("sub", C.c_int32), ("changed", C.c_uint8)]


class MergeResult(C.Structure):
    """snesimage_merge_result: one step of a character reduction."""
    _fields_ = [("error", C.c_double), ("cost", C.c_uint64), ("tile", C.c_uint16), ("donor", C.c_uint16), ("flip", C.c_uint8), ("rank", C.c_uint8),
                ("unique", C.c_uint16)]


class SharedMergeResult(C.Structure):
    """snesimage_shared_merge_result: one step of a set's character reduction."""
    _fields_ = [("error", C.c_double), ("member_error", C.c_double), ("cost", C.c_uint64), ("member", C.c_uint16), ("tile", C.c_uint16),
                ("donor_member", C.c_uint16), ("donor", C.c_uint16), ("unique", C.c_uint16), ("flip", C.c_uint8), ("rank", C.c_uint8), ("pad", C.c_uint8 * 4)]


class RefitResult(C.Structure):
    """snesimage_refit_result: one call of a refit sweep."""
    _fields_ = [("error", C.c_double), ("gain", C.c_uint64), ("rep", C.c_uint16), ("members", C.c_uint16), ("changed", C.c_uint8), ("scored", C.c_uint8),
                ("pad", C.c_uint8 * 2)]


class SharedRefitResult(C.Structure):
    """snesimage_shared_refit_result: one call of a set's refit sweep."""
    _fields_ = [("error", C.c_double), ("gain", C.c_uint64), ("rep", C.c_uint16), ("members", C.c_uint16), ("touched", C.c_uint16), ("changed", C.c_uint8),
                ("scored", C.c_uint8)]


class NativeLayout(C.Structure):
    """snesimage_native_layout: depth and bases of a native export (all zero: auto depth, bases 0)."""
    _fields_ = [("bpp", C.c_uint8), ("palette_base", C.c_uint8), ("priority", C.c_uint8), ("pad", C.c_uint8), ("char_base", C.c_uint16), ("pad2", C.c_uint16)]


class NativeInfo(C.Structure):
    """snesimage_native_info: what a native export produced."""
    _fields_ = [("bpp", C.c_uint32), ("unique", C.c_uint32), ("chr_bytes", C.c_uint32), ("map_words", C.c_uint32)]


# every symbol include/snesimage_hip.h declares: (name, restype, argtypes)
SIGNATURES = [
    ("snesimage_create", C.c_int32, [_u8p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32,
                                     C.POINTER(C.c_void_p)]),
    ("snesimage_destroy", None, [C.c_void_p]),
    ("snesimage_set_stream", C.c_int32, [C.c_void_p, C.c_void_p]),
    ("snesimage_sync", C.c_int32, [C.c_void_p]),
    ("snesimage_set_chunk", C.c_int32, [C.c_void_p, C.c_uint32]),
    ("snesimage_initialize_tiles", C.c_int32, [C.c_void_p]),
    ("snesimage_recalculate_palettes", C.c_int32, [C.c_void_p]),
    ("snesimage_optimize", C.c_int32, [C.c_void_p]),
    ("snesimage_error", C.c_int32, [C.c_void_p, _f64p]),
    ("snesimage_reassign_tiles", C.c_int32, [C.c_void_p, _u32p]),
    ("snesimage_score_tile_moves", C.c_int32, [C.c_void_p, _u16p, _u8p, C.c_uint32, _f64p, _u8p]),
    ("snesimage_tile_step", C.c_int32, [C.c_void_p, C.c_uint32, C.POINTER(TileResult)]),
    ("snesimage_tile_sweep", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(TileResult), C.POINTER(RunStats)]),
    ("snesimage_shared_tile_sweep", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(TileResult), C.POINTER(RunStats)]),
    ("snesimage_set_palette_blocks", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32]),
    ("snesimage_get_palette_blocks", C.c_int32, [C.c_void_p, _u32p, _u32p]),
    ("snesimage_score_block_moves", C.c_int32, [C.c_void_p, _u16p, _u8p, C.c_uint32, _f64p, _u8p]),
    ("snesimage_block_step", C.c_int32, [C.c_void_p, C.c_uint32, C.POINTER(TileResult)]),
    ("snesimage_block_sweep", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(TileResult), C.POINTER(RunStats)]),
    ("snesimage_characters", C.c_int32, [C.c_void_p, _u32p, _u16p, _u8p, _u8p]),
    ("snesimage_merge_shortlist", C.c_int32, [C.c_void_p, C.c_uint32, _u16p, _u16p, _u8p, _u64p, _u32p]),
    ("snesimage_score_merges", C.c_int32, [C.c_void_p, _u16p, _u16p, _u8p, C.c_uint32, _f64p, _u8p]),
    ("snesimage_reduce_characters", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(MergeResult), C.c_uint32, _u32p, _u32p]),
    ("snesimage_as_tilemap_json", C.c_int64, [C.c_void_p, C.c_char_p, C.c_int64]),
    ("snesimage_character_fits", C.c_int32, [C.c_void_p, _u16p, _u16p, _u64p, _u8p, _u32p]),
    ("snesimage_score_refits", C.c_int32, [C.c_void_p, _u16p, C.c_uint32, _f64p, _u8p]),
    ("snesimage_refit_characters", C.c_int32, [C.c_void_p, C.c_uint32, C.POINTER(RefitResult), C.c_uint32, _u32p, _u32p, _u32p, C.POINTER(RunStats)]),
    ("snesimage_shared_characters", C.c_int32, [C.c_void_p, _u32p, _u16p, _u8p, _u8p]),
    ("snesimage_shared_merge_shortlist", C.c_int32, [C.c_void_p, C.c_uint32, _u16p, _u16p, _u16p, _u16p, _u8p, _u64p, _u32p]),
    ("snesimage_shared_score_merges", C.c_int32, [C.c_void_p, _u16p, _u16p, _u16p, _u16p, _u8p, C.c_uint32, _f64p, _u8p]),
    ("snesimage_shared_reduce_characters", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(SharedMergeResult), C.c_uint32, _u32p, _u32p]),
    ("snesimage_shared_as_tilemap_json", C.c_int64, [C.c_void_p, C.c_char_p, C.c_int64]),
    ("snesimage_export_native", C.c_int32, [C.c_void_p, C.POINTER(NativeLayout), _u8p, _u8p, C.c_uint64, _u16p, C.POINTER(NativeInfo)]),
    ("snesimage_shared_export_native", C.c_int32, [C.c_void_p, C.POINTER(NativeLayout), _u8p, _u8p, C.c_uint64, _u16p, C.POINTER(NativeInfo)]),
    ("snesimage_render_native", C.c_int32, [C.c_void_p, C.POINTER(NativeLayout), _u8p, _u8p, C.c_uint64, _u16p, _u8p]),
    ("snesimage_import_native", C.c_int32, [C.c_void_p, C.POINTER(NativeLayout), _u8p, _u8p, C.c_uint64, _u16p, C.POINTER(NativeInfo)]),
    ("snesimage_shared_import_native", C.c_int32, [C.c_void_p, C.POINTER(NativeLayout), _u8p, _u8p, C.c_uint64, _u16p, C.POINTER(NativeInfo)]),
    ("snesimage_shared_character_fits", C.c_int32, [C.c_void_p, _u16p, _u16p, _u64p, _u8p, _u32p]),
    ("snesimage_shared_score_refits", C.c_int32, [C.c_void_p, _u16p, C.c_uint32, _f64p, _f64p, _u8p]),
    ("snesimage_shared_refit_characters", C.c_int32, [C.c_void_p, C.c_uint32, C.POINTER(SharedRefitResult), C.c_uint32, _u32p, _u32p, _u32p, C.POINTER(RunStats)]),
    ("snesimage_score_candidates", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, _u8p, C.c_uint32, _f64p]),
    ("snesimage_score_candidates_device", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                                      C.c_void_p, C.c_void_p]),
    ("snesimage_remap_candidates_device", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    ("snesimage_step", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                   C.c_uint64, C.c_uint32, _f64p, _u8p]),
    ("snesimage_step_async", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                         C.c_uint64, C.c_uint32]),
    ("snesimage_last_step", C.c_int32, [C.c_void_p, _f64p, _u8p, _i32p]),
    ("snesimage_step_begin", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                         C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    ("snesimage_step_commit", C.c_int32, [C.c_void_p, C.c_void_p]),
    ("snesimage_run_slots", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, _u32p, _u32p, _u32p, _u32p, C.c_uint32, C.c_uint32,
                                        C.POINTER(CallResult), C.POINTER(RunStats)]),
    ("snesimage_slots_reserve", C.c_int32, [C.c_void_p, C.c_uint32]),
    ("snesimage_slots_begin", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                          C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, _u32p, _u32p]),
    ("snesimage_slots_commit", C.c_int32, [C.c_void_p, C.c_void_p, _u32p, _u32p, C.POINTER(CallResult)]),
    ("snesimage_group_create", C.c_int32, [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_void_p)]),
    ("snesimage_group_destroy", None, [C.c_void_p]),
    ("snesimage_group_step", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32,
                                         _f64p, _u8p]),
    ("snesimage_group_run_slots", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, _u32p, _u32p, _u32p, _u32p, C.c_uint32, C.c_uint32,
                                              C.POINTER(CallResult), C.POINTER(RunStats)]),
    ("snesimage_batch_create", C.c_int32, [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_void_p)]),
    ("snesimage_batch_destroy", None, [C.c_void_p]),
    ("snesimage_batch_step_async", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64),
                                               C.c_uint64, C.c_uint32]),
    ("snesimage_batch_sync", C.c_int32, [C.c_void_p]),
    ("snesimage_shared_create", C.c_int32, [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_void_p)]),
    ("snesimage_shared_destroy", None, [C.c_void_p]),
    ("snesimage_shared_initialize_tiles", C.c_int32, [C.c_void_p]),
    ("snesimage_shared_recalculate_palettes", C.c_int32, [C.c_void_p]),
    ("snesimage_shared_set_palette_rgb5", C.c_int32, [C.c_void_p, _u8p]),
    ("snesimage_shared_error", C.c_int32, [C.c_void_p, _f64p]),
    ("snesimage_shared_score_candidates", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, _u8p, C.c_uint32, _f64p]),
    ("snesimage_shared_step", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64,
                                          C.c_uint32, _f64p, _u8p]),
    ("snesimage_shared_step_async", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                                C.c_uint64, C.c_uint32]),
    ("snesimage_shared_last_step", C.c_int32, [C.c_void_p, C.POINTER(CallResult)]),
    ("snesimage_shared_reassign_tiles", C.c_int32, [C.c_void_p, _u32p]),
    ("snesimage_shared_run_slots", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, _u32p, _u32p, _u32p, _u32p, C.c_uint32,
                                               C.c_uint32, C.POINTER(CallResult), C.POINTER(RunStats)]),
    ("snesimage_shared_slots_reserve", C.c_int32, [C.c_void_p, C.c_uint32]),
    ("snesimage_shared_create_backdrop", C.c_int32, [C.POINTER(C.c_void_p), C.c_uint32, _u8p, C.POINTER(C.c_void_p)]),
    ("snesimage_shared_get_backdrop_rgb5", C.c_int32, [C.c_void_p, _u8p]),
    ("snesimage_shared_set_backdrop_rgb5", C.c_int32, [C.c_void_p, _u8p]),
    ("snesimage_get_tile_palettes", C.c_int32, [C.c_void_p, _u8p]),
    ("snesimage_set_tile_palettes", C.c_int32, [C.c_void_p, _u8p]),
    ("snesimage_get_palette_rgb5", C.c_int32, [C.c_void_p, _u8p]),
    ("snesimage_set_palette_rgb5", C.c_int32, [C.c_void_p, _u8p]),
    ("snesimage_get_palette_u16", C.c_int32, [C.c_void_p, _u16p]),
    ("snesimage_get_backdrop_rgb5", C.c_int32, [C.c_void_p, _u8p]),
    ("snesimage_set_backdrop_rgb5", C.c_int32, [C.c_void_p, _u8p]),
    ("snesimage_set_ordered_dither", C.c_int32, [C.c_void_p, _i8p, C.c_uint32]),
    ("snesimage_get_ordered_dither", C.c_int32, [C.c_void_p, _i8p, _u32p]),
    ("snesimage_get_target_rgba", C.c_int32, [C.c_void_p, _u8p]),
    ("snesimage_bayer_offsets", None, [C.c_uint32, C.c_uint32, _i8p]),
    ("snesimage_set_ordered_dither_bank", C.c_int32, [C.c_void_p, _i8p, C.c_uint32, C.c_uint32, C.c_uint32]),
    ("snesimage_get_ordered_dither_bank", C.c_int32, [C.c_void_p, _i8p, _u32p, _u32p]),
    ("snesimage_get_tile_levels", C.c_int32, [C.c_void_p, _u8p]),
    ("snesimage_set_tile_levels", C.c_int32, [C.c_void_p, _u8p]),
    ("snesimage_score_tile_levels", C.c_int32, [C.c_void_p, _u16p, _u8p, C.c_uint32, _f64p, _u8p]),
    ("snesimage_level_step", C.c_int32, [C.c_void_p, C.c_uint32, C.POINTER(TileResult)]),
    ("snesimage_level_sweep", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(TileResult), C.POINTER(RunStats)]),
    ("snesimage_shared_set_ordered_dither_bank", C.c_int32, [C.c_void_p, _i8p, C.c_uint32, C.c_uint32, C.c_uint32]),
    ("snesimage_shared_set_tile_levels", C.c_int32, [C.c_void_p, C.c_uint32, _u8p]),
    ("snesimage_shared_score_tile_levels", C.c_int32, [C.c_void_p, _u16p, _u8p, C.c_uint32, _f64p, _f64p]),
    ("snesimage_shared_level_sweep", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(TileResult), C.POINTER(RunStats)]),
    ("snesimage_guided_costs", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, _u64p]),
    ("snesimage_guided_candidates", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, _u8p, _u64p]),
    ("snesimage_guided_step", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, _f64p, _u8p]),
    ("snesimage_guided_step_async", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]),
    ("snesimage_guided_sweep", C.c_int32, [C.c_void_p, C.c_uint32, C.POINTER(CallResult), C.POINTER(RunStats)]),
    ("snesimage_guided_run_slots", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, _u32p, _u32p, C.c_uint32, C.POINTER(CallResult), C.POINTER(RunStats)]),
    ("snesimage_shared_guided_costs", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, _u64p]),
    ("snesimage_shared_guided_candidates", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, _u8p, _u64p]),
    ("snesimage_shared_guided_step", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, _f64p, _u8p]),
    ("snesimage_shared_guided_step_async", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]),
    ("snesimage_shared_guided_sweep", C.c_int32, [C.c_void_p, C.c_uint32, C.POINTER(CallResult), C.POINTER(RunStats)]),
    ("snesimage_shared_guided_run_slots", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, _u32p, _u32p, C.c_uint32, C.POINTER(CallResult), C.POINTER(RunStats)]),
    ("snesimage_set_guided_proxy", C.c_int32, [C.c_void_p, C.c_uint32]),
    ("snesimage_get_guided_proxy", C.c_int32, [C.c_void_p, _u32p]),
    ("snesimage_shared_set_guided_proxy", C.c_int32, [C.c_void_p, C.c_uint32]),
    ("snesimage_shared_get_guided_proxy", C.c_int32, [C.c_void_p, _u32p]),
    ("snesimage_get_palette_map", C.c_int32, [C.c_void_p, _u8p]),
    ("snesimage_set_palette_map", C.c_int32, [C.c_void_p, _u8p]),
    ("snesimage_as_rgba", C.c_int32, [C.c_void_p, _u8p]),
    ("snesimage_as_json", C.c_int64, [C.c_void_p, C.c_char_p, C.c_int64]),
    ("snesimage_random_candidates", None, [C.c_uint64, C.c_uint64, C.c_uint32, _u8p]),
    ("snesimage_schedule_next", None, [C.c_uint32, C.c_uint32, C.c_int32, _u32p, _u32p, _u32p, _u32p, _u32p]),
    ("snesimage_schedule_next_backdrop", None, [C.c_uint32, C.c_uint32, C.c_int32, _u32p, _u32p, _u32p, _u32p, _u32p]),
    ("snesimage_debug_math", C.c_int32, [C.c_int32, C.c_int32, _f32p, _f32p, C.c_uint32, _f32p]),
    ("snesimage_debug_fail_alloc", None, [C.c_int32]),
    ("snesimage_debug_poison_alloc", None, [C.c_int32]),
    ("snesimage_debug_guided_capture", C.c_int32, [C.c_void_p, C.c_int32]),
    ("snesimage_debug_guided_shortlists", C.c_int32, [C.c_void_p, _u8p, C.c_uint32, _u32p, _u32p]),
    ("snesimage_shared_debug_guided_capture", C.c_int32, [C.c_void_p, C.c_int32]),
    ("snesimage_shared_debug_guided_shortlists", C.c_int32, [C.c_void_p, _u8p, C.c_uint32, _u32p, _u32p]),
    ("snesimage_shared_debug_guided_window_costs", C.c_int32, [C.c_void_p, _u32p, _u32p, C.c_uint32, _u64p]),
    ("snesimage_timing_enable", C.c_int32, [C.c_void_p, C.c_int32]),
    ("snesimage_timing_read", C.c_int32, [C.c_void_p, _f64p, _u64p, _u64p]),
    ("snesimage_last_error", C.c_char_p, []),
    ("snesimage_version", C.c_char_p, []),
]

_lib = None


def load():
    """Load libsnesimage_hip.so and type every entry point. Raises if the library is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise ImportError(
                "libsnesimage_hip.so not found at %s: build it with `make -C snesimage_amd/csrc` "
                "(there is no CPU fallback)" % SO_PATH)
        lib = C.CDLL(SO_PATH)
        for name, res, args in SIGNATURES:
            fn = getattr(lib, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib
