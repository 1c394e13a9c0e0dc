/* include/snesimage_hip.h — C ABI of libsnesimage_hip.so, the MI355X (gfx950) implementation of
 * snesimage's palette-optimizer hot path.
 *
 * The reference (aexoden/snesimage, Rust) has no FFI or plugin seam: the hot path is the private
 * method set of `struct OptimizedImage` (/root/reference/src/lib.rs:33-626) called from `run()`
 * (lib.rs:851, 893-910, 988, 1002, 1021).  This header defines that seam as a C ABI; each entry
 * point names the reference method it replaces.  A Rust host binds it with an `extern "C"` block
 * (INTEGRATION.md).  Conventions:
 *   - every function returns 0 on success and a negative code on failure; the message is available
 *     from snesimage_last_error() (thread-local, owned by the library) — the C analogue of the
 *     reference's anyhow::Result + context strings (lib.rs:82, 186, 212 ...; main.rs:16-19);
 *   - snesimage_ctx owns all device memory (the reference struct owns its Vecs, lib.rs:33-43);
 *     the caller owns every pointer it passes; host pointers are copied during the call;
 *   - a ctx is bound to one HIP device and one stream and is not thread-safe (the reference is
 *     single-threaded); independent contexts may be used from different threads;
 *   - there is no CPU fallback: creation fails if no HIP device is usable.
 * Colours cross the boundary as raw 5-bit (r,g,b) byte triples — `SnesColor.data` (lib.rs:629-638)
 * — or as BGR555 words where the reference itself emits them (`as_u16`, lib.rs:679-681).
 */
#ifndef SNESIMAGE_HIP_H
#define SNESIMAGE_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct snesimage_ctx snesimage_ctx;

/* config.rs:20-30 (--dither, --perceptual-palettes, --nes) */
enum { SNES_DITHER = 1, SNES_PERCEPTUAL = 2, SNES_NES = 4 };
/* NOT a reference flag: the shared backdrop colour.  On the SNES a background tile reads index 0 of its subpalette as
 * transparent, and where nothing lies behind the layer the PPU draws the backdrop colour, CGRAM word 0: a picture on the
 * bottom layer has sub_size + 1 colours in every tile, the tile's own and one colour B that all tiles share (the reference
 * writes 0 into slot 0 of every palette row, lib.rs:582-594).  A *backdrop context* (sub_count, sub_size, flags | SNES_BACKDROP)
 * behaves exactly as the EXPANDED context (sub_count, sub_size + 1, flags) whose entries (p, sub_size), p < sub_count, hold B
 * and only ever change together:
 *   - every pixel chooses among its tile's sub_size regular entries and B; B is entry sub_size, so a regular entry wins a
 *     tie (strict <, lowest index, lib.rs:788-791); --dither diffuses against B like against any entry;
 *   - palette_map holds 0 .. sub_size, sub_size meaning backdrop; as_rgba paints such a pixel with B; transparent source
 *     pixels stay (0,0,0,0) and error() treats them as the reference does (lib.rs:527-536);
 *   - get/set_palette_rgb5 and get_palette_u16 keep their size, sub_count*sub_size regular entries; B has its own accessors;
 *   - B starts, in snesimage_create, as the mean of the opaque pixels — per channel (sum + n/2) / n in integers, then >> 3;
 *     (0,0,0) without an opaque pixel — snapped as new_nes_only does (lib.rs:640-660) with SNES_NES.  The initialisers are the
 *     reference's on the regular entries (k-means with k = sub_size) and never move B; their closing optimize() sees it;
 *   - sub_size <= 15 and sub_count*(sub_size + 1) <= 253, else SNES_ERR_ARG;
 *   - THE BACKDROP SLOT is addressed as palette == sub_count, index == 0 in snesimage_score_candidates(_device),
 *     snesimage_remap_candidates_device, snesimage_step(_async), snesimage_step_begin/_commit: a candidate replaces B in
 *     every subpalette at once; the method rules (64 random / the 32 values of one channel of B / the 56 NES colours) and the
 *     acceptance rule (lib.rs:216-219) are those of any entry.  Regular slots are (p < sub_count, i < sub_size); on a context
 *     without the flag palette == sub_count stays SNES_ERR_ARG;
 *   - snesimage_run_slots follows snesimage_schedule_next_backdrop: a window ends in front of a backdrop call, which is
 *     stepped on its own; for every `window` the result equals call by call, bit for bit; log[j].rgb5 of such a call is B;
 *   - snesimage_reassign_tiles, snesimage_score_tile_moves, snesimage_tile_step and snesimage_tile_sweep work as on the
 *     expanded context (B counts as an entry of every subpalette);
 *   - snesimage_as_json: slot 0 of every palette row holds B as a BGR555 word; `tiles` holds 0 for a transparent or a backdrop
 *     pixel, else map + 1;
 *   - snesimage_batch_create, snesimage_group_create, snesimage_shared_create, snesimage_slots_begin and _commit refuse a
 *     backdrop context with SNES_ERR_UNSUPPORTED (their hosts do not carry the backdrop schedule); a shared-palette set of
 *     backdrop contexts is made by snesimage_shared_create_backdrop (below). */
enum { SNES_BACKDROP = 8 };
/* optimizer methods: lib.rs:191 (random), :286 (channel), :242 (nes) */
enum { SNES_METHOD_RANDOM = 0, SNES_METHOD_CHANNEL = 1, SNES_METHOD_NES = 2 };

enum {
    SNES_OK = 0,
    SNES_ERR_ARG = -1,       /* bad argument (sizes, null pointers, slot out of range) */
    SNES_ERR_HIP = -2,       /* a HIP runtime call failed */
    SNES_ERR_STATE = -3,     /* call not valid in the current state */
    SNES_ERR_KMEANS = -4,    /* cogset precondition 2 <= k < n violated (the reference panics) */
    SNES_ERR_UNSUPPORTED = -5
};

/* OptimizedImage::new — lib.rs:46-65.  rgba: w*h*4 bytes, row-major RGBA8.  w must be 256 (tile
 * stride hard-coded to 32, lib.rs:58,565); h a multiple of 8 in [8,256] (256 x 224, the SNES frame, included; a
 * 239-row picture is padded to 240 by the caller).  sub_count*sub_size <= 253.
 * device: HIP device ordinal (>= 0). */
int32_t snesimage_create(const uint8_t *rgba, uint32_t w, uint32_t h, uint32_t sub_count,
                         uint32_t sub_size, uint32_t flags, int32_t device, snesimage_ctx **out);
void snesimage_destroy(snesimage_ctx *ctx);

/* Plumbing: run all subsequent work on an existing hipStream_t (e.g. torch's current stream).
 * NULL restores the context's own stream. */
int32_t snesimage_set_stream(snesimage_ctx *ctx, void *hip_stream);
/* Block until all work queued by this context has finished. */
int32_t snesimage_sync(snesimage_ctx *ctx);
/* Most candidates one internal launch group takes (bounds the workspace, which grows on demand);
 * default 4096.  A candidate list is split evenly over the context's launch lanes up to this bound. */
int32_t snesimage_set_chunk(snesimage_ctx *ctx, uint32_t chunk);

int32_t snesimage_initialize_tiles(snesimage_ctx *ctx);     /* lib.rs:79-189  */
int32_t snesimage_recalculate_palettes(snesimage_ctx *ctx); /* lib.rs:407-415 */
int32_t snesimage_optimize(snesimage_ctx *ctx);             /* lib.rs:425-501 */
int32_t snesimage_error(snesimage_ctx *ctx, double *out);   /* lib.rs:503-548 */

/* The loop body of lib.rs:205-220 / 252-262 / 296-306 for an explicit candidate list: for each
 * k < n, entry (palette,index) := rgb5[3k..3k+2], optimize(), error() -> errors[k].  The context's
 * palette and palette_map are left unchanged.  Host pointers; synchronous. */
int32_t snesimage_score_candidates(snesimage_ctx *ctx, uint32_t palette, uint32_t index,
                                   const uint8_t *rgb5, uint32_t n, double *errors);
/* Same with device pointers, asynchronous on the context's stream (no host synchronisation).
 * maps_out (optional, device, n*w*h bytes) receives each candidate's palette_map. */
int32_t snesimage_score_candidates_device(snesimage_ctx *ctx, uint32_t palette, uint32_t index,
                                          const uint8_t *d_rgb5, uint32_t n, double *d_errors,
                                          uint8_t *d_maps_out);
/* The remap alone — the optimize() of lib.rs:210-213 for each candidate, without its error():
 * d_maps_out (device, n*w*h bytes) receives the palette_map each candidate would produce.
 * Device pointers, asynchronous on the context's stream. */
int32_t snesimage_remap_candidates_device(snesimage_ctx *ctx, uint32_t palette, uint32_t index,
                                          const uint8_t *d_rgb5, uint32_t n, uint8_t *d_maps_out);

/* One optimizer call — optimize_palette_entry_{random,channel,nes} (lib.rs:191-328) followed by
 * lib.rs:906-910.  Random candidates come from the counter RNG keyed (seed, step_id);
 * n_random = 0 means the reference's 64 (lib.rs:205).  best_error / best_rgb5 may be NULL. */
int32_t snesimage_step(snesimage_ctx *ctx, uint32_t method, uint32_t palette, uint32_t index,
                       uint32_t channel, uint64_t seed, uint64_t step_id, uint32_t n_random,
                       double *best_error, uint8_t *best_rgb5);
/* The same without any host synchronisation; results via snesimage_last_step(). */
int32_t snesimage_step_async(snesimage_ctx *ctx, uint32_t method, uint32_t palette, uint32_t index,
                             uint32_t channel, uint64_t seed, uint64_t step_id, uint32_t n_random);
int32_t snesimage_last_step(snesimage_ctx *ctx, double *best_error, uint8_t *best_rgb5,
                            int32_t *best_k);

/* Split-phase step for candidate sharding across GPUs.  Phase 1 scores the
 * candidates k with k % shard_count == shard_rank of the n_total candidates of this call and
 * writes d_errors[k] (device, n_total doubles; +inf for candidates owned by other ranks).  The
 * caller min-all-reduces d_errors across ranks (RCCL), then phase 2 applies the reference's
 * acceptance rule (strict <, ascending k, lib.rs:216-219) identically on every rank. */
int32_t snesimage_step_begin(snesimage_ctx *ctx, uint32_t method, uint32_t palette, uint32_t index,
                             uint32_t channel, uint64_t seed, uint64_t step_id, uint32_t n_total,
                             uint32_t shard_rank, uint32_t shard_count, double *d_errors);
int32_t snesimage_step_commit(snesimage_ctx *ctx, const double *d_errors);

/* Speculative multi-slot stepping — the reference's own loop (lib.rs:888-933: one call of optimize_palette_entry_random
 * with 64 candidates, lib.rs:191-240, or _channel with 32, lib.rs:286-328, or _nes with 56, lib.rs:242-284, per scheduler
 * slot), several calls per launch.  Call j+1 of that loop sees the state call j saw whenever call j accepted nothing
 * (strict <, lib.rs:216-219), so a *window* scores the next K calls of the schedule against the current palette in one set
 * of launches, applies their decisions in order and stops behind the first call that changed the state; the calls behind
 * it are void and are scored again by the next window.  Bit-identical to snesimage_schedule_next + snesimage_step per
 * call, for every K.  Windows cover the group-sparse path (every height since round 4; with --dither, subpalettes of two entries and more);
 * what is left — one-entry subpalettes with --dither, a library run with SNES_SPARSE=0 — is stepped call by call inside snesimage_run_slots. */
typedef struct { double error; int32_t best_k; uint8_t rgb5[3]; uint8_t changed; } snesimage_call_result; /* what snesimage_last_step reports after the call */
typedef struct {
    uint32_t calls, accepted, windows, voided;   /* calls that took effect; calls that changed the palette; launch sets collected;
                                                  * launch sets enqueued ahead and voided on the device (they scored nothing) */
    uint64_t scored, useful;                     /* candidates scored in all; candidates of the calls that took effect */
} snesimage_run_stats;
/* n_calls calls from scheduler state (*palette, *index, *channel, *step) — advanced as by snesimage_schedule_next — call j
 * drawing its random candidates from stream (seed, first_step_id + j); n_random = 0: the reference's 64 (lib.rs:205), at most 64
 * in a window (larger calls are stepped one by one).  window: calls per launch set (0 = adaptive: the size that
 * gets most calls through per unit of time at the acceptance rate of the recent windows, at most SNES_WINDOW_MAX, default 64;
 * 1 = call by call).
 * log (optional): n_calls records.  stats (optional). */
int32_t snesimage_run_slots(snesimage_ctx *ctx, uint32_t n_calls, uint64_t seed, uint64_t first_step_id, uint32_t *palette,
                            uint32_t *index, uint32_t *channel, uint32_t *step, uint32_t n_random, uint32_t window,
                            snesimage_call_result *log, snesimage_run_stats *stats);
/* Allocate the storage of windows of up to n_slots calls now instead of on first use (about 0.3 GB of HBM per call; the
 * library never takes more than SNES_WINDOW_MAX, default 64, calls per window). */
int32_t snesimage_slots_reserve(snesimage_ctx *ctx, uint32_t n_slots);
/* The two phases of one window, for sharding its calls over GPUs (the window's calls in runs of six consecutive calls, round robin over the ranks: every call its own base
 * image, its own candidates).  Phase 1 takes at most n_slots calls from the given scheduler state — fewer where the method
 * changes, all calls of a window having the same number of candidates (*stride) — and writes errors[j * stride + k]
 * (device, n_slots * 64 doubles; +inf for calls of other ranks; NULL = the context's own vector, single rank only);
 * n_slots is capped at SNES_WINDOW_MAX * shard_count (and 1024).  The
 * caller min-all-reduces the first *n_taken * *stride doubles, then phase 2 commits identically on every rank: *consumed
 * calls took effect, *accepted = the last of them changed the palette; log (host, optional): *n_taken records. */
int32_t snesimage_slots_begin(snesimage_ctx *ctx, uint32_t n_slots, uint64_t seed, uint64_t first_step_id, uint32_t palette,
                              uint32_t index, uint32_t channel, uint32_t step, uint32_t n_random, uint32_t shard_rank,
                              uint32_t shard_count, double *d_errors, uint32_t *n_taken, uint32_t *stride);
int32_t snesimage_slots_commit(snesimage_ctx *ctx, const double *d_errors, uint32_t *consumed, uint32_t *accepted,
                               snesimage_call_result *log);

/* One process, several GPUs: a group borrows one context per device, all created from the same image and brought to
 * the same state (initialise one, copy tile_palettes and palette to the others, optimize()).  snesimage_group_step is
 * snesimage_step with the candidates sharded over the members (rank r scores k = r mod N): step_begin on every member,
 * one grouped RCCL all-reduce(min) of the error vectors on the members' streams, step_commit on every member — the
 * palettes stay bit-identical on all devices.  n_total as in snesimage_step_begin.  librccl is opened at run time.
 * Lifetime: the group borrows its contexts — destroy the group first.  Destroying a member first retires the group
 * (snesimage_group_step then fails with SNES_ERR_STATE; snesimage_group_destroy is still required).  A context belongs
 * to at most one group.  A failed step leaves no member with a pending split-phase step. */
typedef struct snesimage_group snesimage_group;
int32_t snesimage_group_create(snesimage_ctx **ctxs, uint32_t n, snesimage_group **out);
void snesimage_group_destroy(snesimage_group *group);
int32_t snesimage_group_step(snesimage_group *group, uint32_t method, uint32_t palette, uint32_t index,
                             uint32_t channel, uint64_t seed, uint64_t step_id, uint32_t n_total,
                             double *best_error, uint8_t *best_rgb5 /*3*/);

/* snesimage_run_slots over a group: the calls of every window are dealt to the members (runs of six consecutive calls, round robin), one grouped
 * RCCL all-reduce(min) over the window's error vector, identical in-order commit on every member.  Same arguments, same
 * trajectory (lib.rs:888-933), bit-identical palettes on all devices.  Every member must be in the state
 * snesimage_group_create asks for. */
int32_t snesimage_group_run_slots(snesimage_group *group, uint32_t n_calls, uint64_t seed, uint64_t first_step_id,
                                  uint32_t *palette, uint32_t *index, uint32_t *channel, uint32_t *step, uint32_t n_random, uint32_t window,
                                  snesimage_call_result *log, snesimage_run_stats *stats);

/* Throughput mode — many independent images on one device, one launch per stage of an optimizer call
 * for all of them (the reference runs one image per process: `run()` lib.rs:830-1024 once per file).
 * A batch borrows its contexts (same device, image size, palette geometry, chunk and flags — either distance, with or
 * without --dither): snesimage_batch_step_async is snesimage_step_async for every member — same slot and
 * method, candidate stream of member i keyed (seeds[i], step_id), at most `chunk` candidates — enqueued
 * on the batch's stream.  Any other call on a member context first waits for that stream, and the first batched call
 * after such a call waits for the member's own stream; snesimage_set_chunk is refused on a lent context.  The batch does
 * not own the contexts: destroy it before them (destroying a member first retires the batch: later calls fail with
 * SNES_ERR_STATE). */
typedef struct snesimage_batch snesimage_batch;
int32_t snesimage_batch_create(snesimage_ctx **ctxs, uint32_t n, snesimage_batch **out);
void snesimage_batch_destroy(snesimage_batch *batch);
int32_t snesimage_batch_step_async(snesimage_batch *batch, uint32_t method, uint32_t palette, uint32_t index,
                                   uint32_t channel, const uint64_t *seeds /*n*/, uint64_t step_id,
                                   uint32_t n_random);
int32_t snesimage_batch_sync(snesimage_batch *batch);

/* One palette shared by several images — the frames of an animated background, the poses of a sprite: on the SNES everything
 * drawn on one background reads the same CGRAM (the reference optimizes one image per process, lib.rs:833-853).  A set borrows
 * F >= 1 contexts (members) as a batch does — same device, image size, palette geometry, chunk and flags; a member belongs to
 * no batch, group or other set — and keeps one palette in all of them; each member keeps its own tile_palettes and
 * palette_map.  The set's error is E = sum of the members' error() in member order (binary64, left to right).
 * An optimizer call gives every member the same candidate list (random: keyed (seed, step_id) as in snesimage_step; channel,
 * NES: from the shared palette), E_k = sum of the members' e_{i,k}, and the reference's acceptance rule on E (strict < against
 * the members' summed incumbents, lib.rs:216-219; the NES method takes its argmin, lib.rs:250): the winner goes to every
 * member, whose incumbent becomes its own e_{i,k*}.  A set of one member steps exactly as snesimage_step.
 * The initialisers are the reference's own on the member stack (the members top to bottom in member order, W x F*H): tile
 * means in its order over that picture (tile_x outer), k-means, the stack's tile palettes split back by rows; the pixels
 * of every tile using subpalette p, member after member.  Then optimize() on every member.
 * snesimage_shared_create refuses members whose palettes differ (SNES_ERR_STATE) and what a batch refuses (SNES_ERR_ARG,
 * SNES_ERR_STATE, SNES_ERR_UNSUPPORTED).  Every set call needs the members as the set left them: a member changed through
 * its own calls (palette, tile palettes, map, a step) makes the next set call fail with SNES_ERR_STATE.  Lifetime as a
 * batch's: destroy the set before its members; destroying a member first retires the set (SNES_ERR_STATE;
 * snesimage_shared_destroy is still required).  Each member's storage is sized for `chunk` candidates (about 4.45 MB per
 * candidate): set the chunk to the call's candidate count before creating the set. */
typedef struct snesimage_shared snesimage_shared;
int32_t snesimage_shared_create(snesimage_ctx **ctxs, uint32_t n, snesimage_shared **out);
void snesimage_shared_destroy(snesimage_shared *set);
int32_t snesimage_shared_initialize_tiles(snesimage_shared *set);     /* lib.rs:79-189 on the member stack */
int32_t snesimage_shared_recalculate_palettes(snesimage_shared *set); /* lib.rs:407-415 on the member stack */
/* the palette of every member := in (count*size*3 raw 5-bit colours), then optimize() on every member */
int32_t snesimage_shared_set_palette_rgb5(snesimage_shared *set, const uint8_t *in);
int32_t snesimage_shared_error(snesimage_shared *set, double *out); /* E */
/* E_k for k < n: snesimage_score_candidates on every member, summed in member order.  Host pointers; synchronous; the
 * members are left unchanged. */
int32_t snesimage_shared_score_candidates(snesimage_shared *set, uint32_t palette, uint32_t index, const uint8_t *rgb5,
                                          uint32_t n, double *errors);
/* One optimizer call on the set (at most `chunk` candidates).  error: E after the call; best_rgb5: the slot's colour. */
int32_t snesimage_shared_step(snesimage_shared *set, uint32_t method, uint32_t palette, uint32_t index, uint32_t channel,
                              uint64_t seed, uint64_t step_id, uint32_t n_random, double *error, uint8_t *best_rgb5);
/* The same without any host synchronisation; results via snesimage_shared_last_step (error = E). */
int32_t snesimage_shared_step_async(snesimage_shared *set, uint32_t method, uint32_t palette, uint32_t index,
                                    uint32_t channel, uint64_t seed, uint64_t step_id, uint32_t n_random);
int32_t snesimage_shared_last_step(snesimage_shared *set, snesimage_call_result *out);
/* snesimage_reassign_tiles on every member (a tile's cost depends on its own pixels and the shared palette only);
 * *moved = tiles moved in all members. */
int32_t snesimage_shared_reassign_tiles(snesimage_shared *set, uint32_t *moved);
/* snesimage_run_slots for a set: the reference's loop for n_calls calls, several calls per launch set.  A window scores the
 * coming K calls for every member against the current palette (a slot context per member and call, about 0.3 GB each),
 * sums the members' errors in member order and commits the calls in schedule order up to the first one that accepts; the
 * rest of the window is scored again.  For every `window` (0 = chosen by the library, 1 = call by call, K = at most K calls
 * per launch set) everything observable afterwards equals snesimage_schedule_next + snesimage_shared_step per call, bit for
 * bit: the shared palette, every member's palette_map, incumbent error and snesimage_last_step, the set's
 * snesimage_shared_last_step, the scheduler state and every log record (log[j].error = E after call j).  Arguments as
 * snesimage_run_slots.  stats count candidates per member: `scored` and `useful` are calls times candidates per call.
 * F members times K calls stay within SNES_WINDOW_MAX (default 64) slot contexts, so K <= SNES_WINDOW_MAX / F; a set of
 * more than SNES_WINDOW_MAX / 2 members, `window` = 1 and n_random > 64 are stepped call by call inside the function.
 * Refusals as every set call: a retired set or a member changed outside the set give SNES_ERR_STATE. */
int32_t snesimage_shared_run_slots(snesimage_shared *set, uint32_t n_calls, uint64_t seed, uint64_t first_step_id,
                                   uint32_t *palette, uint32_t *index, uint32_t *channel, uint32_t *step, uint32_t n_random,
                                   uint32_t window, snesimage_call_result *log, snesimage_run_stats *stats);
/* Slot contexts for windows of up to n_slots calls (clamped to SNES_WINDOW_MAX / F) now rather than on first use.
 * Allocation is grow-only; a failed allocation returns SNES_ERR_HIP and leaves the set usable. */
int32_t snesimage_shared_slots_reserve(snesimage_shared *set, uint32_t n_slots);

/* THE BACKDROP COLOUR OF A SET (DESIGN 5c'').  The frames of one background read the same CGRAM word 0, so a set can carry B:
 * every member is a SNES_BACKDROP context — the expanded context (sub_count, sub_size + 1) with a tied last column — and the set
 * keeps one B in all of them, as it keeps one palette.  snesimage_shared_create_backdrop takes SNES_BACKDROP members only
 * (a plain member: SNES_ERR_ARG, the message names snesimage_shared_create, which takes those); their REGULAR entries must agree
 * (SNES_ERR_STATE), B of every member is then written by the set: backdrop_rgb5 (three 5-bit values; > 31: SNES_ERR_ARG) when
 * given, else snesimage_create's rule on the member stack — per channel (sum over the opaque pixels of all members + n/2) / n in
 * integers, n = their count, then >> 3; snapped to the table with SNES_NES; (0,0,0) without an opaque pixel.  Everything else a
 * set refuses is refused here; snesimage_shared_create, snesimage_batch_create and snesimage_group_create keep refusing backdrop
 * members.  On such a set:
 *   - snesimage_shared_step(_async) and snesimage_shared_score_candidates take the backdrop slot (palette == sub_count,
 *     index == 0): a candidate replaces B in every subpalette of every member, E_k = sum of the members' e_{i,k} in member
 *     order, the acceptance rule is that of any set call; the winner goes to all tied entries of all members.  A set of one
 *     steps exactly as snesimage_step on a backdrop context;
 *   - snesimage_shared_run_slots follows snesimage_schedule_next_backdrop (a window ends in front of a backdrop call, which is
 *     stepped on its own), bit-identical to call by call for every `window`;
 *   - the initialisers are the reference's on the member stack at (sub_count, sub_size) and never move B;
 *   - snesimage_shared_set_palette_rgb5 takes the sub_count*sub_size regular entries and leaves B; B has the pair below (the
 *     setter behaves as snesimage_shared_set_palette_rgb5: optimize() on every member afterwards);
 *   - snesimage_shared_error, _reassign_tiles and _tile_sweep work as on the expanded members;
 *   - the character budget, the refit, the set tilemap and the per-tile dither levels of a set (snesimage_shared_characters,
 *     _merge_shortlist, _score_merges, _reduce_characters, _character_fits, _score_refits, _refit_characters, _as_tilemap_json,
 *     _set_ordered_dither_bank, _set_tile_levels, _score_tile_levels, _level_sweep) answer SNES_ERR_UNSUPPORTED and leave the
 *     set usable. */
int32_t snesimage_shared_create_backdrop(snesimage_ctx **ctxs, uint32_t n, const uint8_t *backdrop_rgb5 /*3, may be NULL*/,
                                         snesimage_shared **out);
int32_t snesimage_shared_get_backdrop_rgb5(snesimage_shared *set, uint8_t *out /*3*/);
int32_t snesimage_shared_set_backdrop_rgb5(snesimage_shared *set, const uint8_t *in /*3*/);

/* Dynamic tile -> subpalette reassignment — NOT a reference method: /root/reference/TODO.md:36-37 lists it as missing ("no
 * attempt is made to reassign tiles dynamically if it could improve the overall result").  Every tile with an opaque pixel
 * moves to the subpalette with the strictly smallest cost, cost(p) = sum over the tile's opaque pixels (raster order) of the
 * distance optimize() minimises (lib.rs:1080-1100) to the nearest entry of subpalette p, in binary64; ties keep the current
 * subpalette, then the lower index.  Palettes are kept; optimize() re-runs if a tile moved.  *moved = tiles moved.
 * Refused (SNES_ERR_STATE) between the two phases of a split-phase step.  On the members of a group call it on every
 * member (the result is deterministic: the replicas stay identical), never on one alone. */
int32_t snesimage_reassign_tiles(snesimage_ctx *ctx, uint32_t *moved);

/* Tile moves decided by the objective — NOT a reference method either.  Tiles are numbered as tile_palettes is indexed
 * (t = ty * 32 + tx).  A TILE CALL on tile t, whose subpalette is cur: for k = 0 .. sub_count - 1 ascending, k != cur:
 * tile_palettes[t] := k, optimize(), e_k := error(); acceptance is lib.rs:216-219 (best := incumbent error; e_k < best, strict,
 * takes best := e_k).  If some k was taken the state becomes that candidate's (tile_palettes[t], its palette_map, the incumbent
 * error); otherwise it is untouched bit for bit.  The palette never changes.  With --dither optimize() is the whole
 * Floyd-Steinberg run, so a move may change pixels to the right of and below the tile.  A tile without an opaque pixel and a
 * move between subpalettes that render the tile identically give e_k == incumbent exactly and are never taken.
 * A TILE SWEEP over first_tile, n_tiles is the tile calls on those tiles in that order, each seeing the state the one before
 * left.  snesimage_reassign_tiles moves tiles by a proxy (colour distance, no dithering) that disagrees with the objective:
 * applied after a sweep it moves the tiles back.  Use one or the other in a run.
 * All candidates are scored in batches by the map-reading scorer (every distance, --dither, every height and geometry).
 * Refusals: null context, first_tile + n_tiles beyond (w/8)*(h/8), subs[j] >= sub_count: SNES_ERR_ARG; between the two phases
 * of a split-phase step: SNES_ERR_STATE; a failed workspace allocation: SNES_ERR_HIP, the context usable and unchanged.  On
 * the members of a group the rule of snesimage_reassign_tiles holds. */
typedef struct { double error; int32_t sub; uint8_t changed; } snesimage_tile_result; /* incumbent error and the tile's subpalette after the call */
/* e_j for n explicit (tile, subpalette) pairs against the current state, which is left unchanged.  A pair naming the tile's
 * current subpalette returns the incumbent error bit for bit.  maps_out (optional, n*w*h bytes): each candidate's palette_map.
 * Host pointers; synchronous.  n may exceed the chunk (launch groups as in snesimage_score_candidates, at most 512 pairs each). */
int32_t snesimage_score_tile_moves(snesimage_ctx *ctx, const uint16_t *tiles, const uint8_t *subs, uint32_t n,
                                   double *errors, uint8_t *maps_out);
/* One tile call. */
int32_t snesimage_tile_step(snesimage_ctx *ctx, uint32_t tile, snesimage_tile_result *out);
/* A tile sweep, several tile calls per launch set: a window scores the candidates of the coming K calls against the image as
 * it stands in one batch, commits the calls in order on the device up to the first that accepts, and the calls behind it
 * are scored again by the next window (one synchronisation per window).  window: 0 = chosen by the library, 1 = call by
 * call, K = at most K calls per launch set.  For every window everything observable afterwards equals tile call after tile
 * call, bit for bit.  log (optional): n_tiles records.  stats (optional): as snesimage_run_slots (voided = 0). */
int32_t snesimage_tile_sweep(snesimage_ctx *ctx, uint32_t first_tile, uint32_t n_tiles, uint32_t window,
                             snesimage_tile_result *log, snesimage_run_stats *stats);
/* The same on every member of a set, member after member: a tile move in member i changes e_i alone, so each call is decided
 * on the member's own error (strict < on e_i, not on the rounded sum E) — exactly snesimage_tile_sweep on each member.
 * log: F * n_tiles records, member-major; stats summed over the members. */
int32_t snesimage_shared_tile_sweep(snesimage_shared *set, uint32_t first_tile, uint32_t n_tiles, uint32_t window,
                                    snesimage_tile_result *log, snesimage_run_stats *stats);

/* Palette blocks — NOT a reference method.  Only an SNES background in 8 x 8 tile mode chooses a subpalette per tile: the NES
 * attribute table and an SNES background in 16 x 16 tile mode choose one per 2 x 2 tiles, an OBJ one per 16 x 16, 32 x 32 or
 * 64 x 64 object.  snesimage_set_palette_blocks(ctx, bw, bh) makes the context choose per BLOCK of bw x bh tiles, bw and bh each
 * one of 1, 2, 4, 8, bh dividing h/8.  Block b = by * (32/bw) + bx covers tiles tx in [bx*bw, (bx+1)*bw), ty in
 * [by*bh, (by+1)*bh).  1 x 1, the default, switches blocking off: every launch is then what it is without this section.
 *   THE INVARIANT.  On a context with bw*bh > 1 ("blocked") tile_palettes is constant over every block of the image, always.
 *   The setter changes nothing else (map, incumbent and epoch stay); it checks the current table and refuses with SNES_ERR_STATE
 *   if it is not constant over the new blocks — set such a table first, or call the setter before snesimage_initialize_tiles (a
 *   fresh context, all zeros, passes).  Other refusals: SNES_ERR_ARG for a null context, other values, a bh that does not divide
 *   h/8; SNES_ERR_STATE for a pending split-phase step or window and a context lent to a set, batch or group.
 * On a blocked context:
 *   - snesimage_set_tile_palettes with a table that is not constant over the image's blocks is SNES_ERR_ARG, the message names
 *     the lowest offending block, the context is untouched; entries behind the image's tiles are not judged;
 *   - snesimage_initialize_tiles is lib.rs:79-189 with the block in place of the tile: the outer loops run bx outer, by inner
 *     (the order of the k-means points, so the starting centres); per block the f32 sums and the count run over its opaque
 *     pixels, x outer, y inner over bw*8 x bh*8 pixels, one ordered chain; the test sum[0] + sum[1] + sum[2] > 0 is the block's;
 *     the mean is f64(sum) / f64(count); every tile of a clustered block takes the cluster's index, a block left out keeps
 *     what it had; centre -> colour, the fill and the closing optimize() are unchanged; cogset's 2 <= k < n counts blocks
 *     (SNES_ERR_KMEANS); sub_count == 1 is unchanged;
 *   - snesimage_reassign_tiles moves blocks: cost(b, p) = the binary64 sum, over the block's tiles in raster order (ty outer, tx
 *     inner), of the tile costs defined above, tiles without an opaque pixel contributing nothing; a block with an opaque pixel
 *     moves as a whole by the same rule (strictly smallest, ties keep the current subpalette, then the lower index); *moved
 *     counts tiles, a multiple of bw*bh;
 *   - snesimage_score_tile_moves, snesimage_tile_step and snesimage_tile_sweep answer SNES_ERR_UNSUPPORTED (a single-tile move
 *     would break the invariant; the message names the block call to use), snesimage_import_native likewise, and
 *     snesimage_batch_create, snesimage_group_create, snesimage_shared_create and snesimage_shared_create_backdrop refuse a
 *     blocked member with SNES_ERR_UNSUPPORTED;
 *   - everything else reads tile_palettes and never writes it, so it works unchanged and leaves the table as it found it:
 *     steps, snesimage_run_slots, guided calls and sweeps, snesimage_recalculate_palettes, the backdrop slot, ordered dither
 *     and level sweeps, the character budget, refit and tilemap JSON, snesimage_export_native and snesimage_render_native
 *     (characters stay 8 x 8 cells).
 * BLOCK MOVES decided by the objective are the tile call and the tile sweep above with "tile_palettes[t] := k" read as "every
 * tile of block b := k": ascending k != cur (cur = the block's subpalette), optimize(), error(), strict < against the
 * incumbent, the state of the winning candidate taken whole; a pair naming the block's current subpalette returns the incumbent
 * bit for bit; with --dither a candidate is the whole Floyd-Steinberg run under its own tile table.  They work on every
 * context: at 1 x 1 a block is a tile and the three calls equal the tile calls bit for bit.  Windows, stats, log and refusals
 * are those of snesimage_tile_sweep with blocks for tiles (a block beyond the image's (32/bw)*((h/8)/bh): SNES_ERR_ARG). */
int32_t snesimage_set_palette_blocks(snesimage_ctx *ctx, uint32_t bw, uint32_t bh);
int32_t snesimage_get_palette_blocks(snesimage_ctx *ctx, uint32_t *bw, uint32_t *bh);
int32_t snesimage_score_block_moves(snesimage_ctx *ctx, const uint16_t *blocks, const uint8_t *subs, uint32_t n,
                                    double *errors, uint8_t *maps_out);
int32_t snesimage_block_step(snesimage_ctx *ctx, uint32_t block, snesimage_tile_result *out);
int32_t snesimage_block_sweep(snesimage_ctx *ctx, uint32_t first_block, uint32_t n_blocks, uint32_t window,
                              snesimage_tile_result *log, snesimage_run_stats *stats);

/* The character budget — NOT a reference method.  The JSON gives every tile its own 64 indices; the SNES has 64 KB of VRAM for
 * all layers, and a 256 x 224 picture of 896 distinct 4bpp characters takes 28 KB of it.  These calls count the distinct
 * characters of the result, merge tiles until at most N are left — each merge chosen by error() itself — and write the tilemap
 * the merges imply.  Off unless called; no other entry point changes.  All quantities are integers except the objective.
 * Tiles are numbered as tile_palettes is indexed (t = ty * 32 + tx, ty < h/8; ntile = 32 * h/8).
 *   CHARACTER of tile t: 64 bytes, row-major inside the tile, the values snesimage_as_json writes into `tiles`: 0 where the
 *     source alpha is 0; 0 where, in a backdrop context, the map value is the backdrop; map + 1 otherwise.
 *   FLIP f in 0..3, bit 0 horizontal, bit 1 vertical (bits 14 and 15 of the tilemap word):
 *     flip_f(c)[y][x] = c[y ^ (f & 2 ? 7 : 0)][x ^ (f & 1 ? 7 : 0)].
 *   SAME CHARACTER: c_t == flip_f(c_u) for some f — an equivalence, the flips being a group.  rep(t) is the lowest tile index
 *     of t's class, flip_of(t) the lowest f with c_t == flip_f(c_rep(t)), U the number of classes.  Subpalettes play no part:
 *     the tilemap entry selects the palette, so tiles of different subpalettes with equal index patterns share a character.
 *   PINNED TILE: one with a pixel of source alpha 0.  It is never changed and never donates (the library has no map value for
 *     "transparent", so a merge across such a tile could not be drawn as the hardware draws it).  Pinned tiles count in U; all
 *     fully transparent tiles form one class.
 *   MERGE CANDIDATE (t, b, f), t != b, both unpinned: for every pixel (x, y) of t, map(t; x, y) := map(b; x ^ .., y ^ ..),
 *     flipped as above.  tile_palettes is untouched — t keeps its subpalette and takes b's INDICES — and nothing else changes.
 *     Its ERROR is error() of that stored map: no optimize(), no re-dither.  Its PROXY COST is the sum over t's 64 pixels of
 *     red_mean_key(original pixel, 8-bit expansion of entry (tile_palettes[t], new map value)), the exact integer key of
 *     lib.rs:1080-1088 without the square root, in a uint64_t (below 2^37).  The proxy reads the ORIGINAL image, not an
 *     ordered-dither target, and is this integer key whatever SNES_PERCEPTUAL says; a backdrop map value takes B.  The proxy
 *     only shortlists; the objective decides.
 *   ONE REDUCTION STEP with shortlist length K: recipients are the unpinned tiles that are ALONE in their class (a character
 *     already shared is kept); a recipient's donors are the class representatives that are unpinned and not the recipient.
 *     The shortlist is the K candidates lowest in (cost, t, b, f), compared lexicographically — fewer if fewer exist.  All of
 *     it is scored; the winner is the lowest (error, rank in the shortlist), a NaN never wins.  The winner is applied
 *     UNCONDITIONALLY — a budget is a constraint, there is no comparison with the incumbent.  Afterwards the map is the
 *     candidate's, the incumbent error is the candidate's scored bits and U has fallen by exactly one.
 *   REDUCTION to max_unique: steps while U > max_unique and a recipient with a donor exists.  Running out of eligible pairs is
 *     no error: SNES_OK, and the U that was reached is reported.  Exact duplicates cost nothing: they are one class when U is
 *     first counted.
 *   STATE AFTERWARDS: as after snesimage_set_palette_map, with the error known: the map is a stored map, which error(), as_rgba
 *     and as_json read; the epoch advances.  Every call that re-runs optimize() replaces it — steps, windows,
 *     snesimage_reassign_tiles, tile moves, the palette, tile-palette, backdrop and table setters followed by optimize().
 *     REDUCTION IS THEREFORE THE LAST STAGE OF A RUN.
 * The default shortlist length, 16, is a choice, not a measurement.
 * Refusals: SNES_ERR_ARG for a null context, a tile beyond the image, a pinned tile named explicitly, t == b, f > 3,
 * max_unique == 0, shortlist > 64; SNES_ERR_STATE between the phases of a split-phase step or window and on a context lent to a
 * batch, a set or a group; SNES_ERR_HIP after a failed workspace allocation, the context usable and unchanged. */
typedef struct { double error; uint64_t cost; uint16_t tile, donor; uint8_t flip, rank; uint16_t unique; } snesimage_merge_result; /* 24 bytes; unique = U after the step */
/* U, and optionally rep (ntile), flip_of (ntile) and the characters (ntile * 64) of the image as it stands. */
int32_t snesimage_characters(snesimage_ctx *ctx, uint32_t *unique, uint16_t *rep /*ntile, opt*/, uint8_t *flip /*ntile, opt*/,
                             uint8_t *chars /*ntile*64, opt*/);
/* The shortlist a reduction step with length k (1..64, 0 = 16) would score, in rank order; *n = min(k, candidates that exist).
 * Output arrays (each optional) hold k entries.  The state is unchanged. */
int32_t snesimage_merge_shortlist(snesimage_ctx *ctx, uint32_t k, uint16_t *tiles, uint16_t *donors, uint8_t *flips,
                                  uint64_t *costs, uint32_t *n);
/* errors[j] of n explicit candidates (tiles[j], donors[j], flips[j]) — any unpinned pair, not only recipients and donors —
 * against the current state, which is left unchanged.  A candidate that changes nothing returns the incumbent error bit for
 * bit.  maps_out (optional, n*w*h bytes): each candidate's palette_map.  Host pointers; synchronous; n may exceed the chunk
 * (launch groups as in snesimage_score_tile_moves). */
int32_t snesimage_score_merges(snesimage_ctx *ctx, const uint16_t *tiles, const uint16_t *donors, const uint8_t *flips,
                               uint32_t n, double *errors, uint8_t *maps_out /*opt, n*w*h*/);
/* The reduction.  log (optional): the first log_cap steps' records; *merges: steps taken; *unique: U afterwards.  A budget
 * already met takes no step and leaves the state untouched bit for bit.  If a step fails (SNES_ERR_HIP) the steps before it
 * stand: *merges and *unique report them, and the map is a stored map whose error is recomputed when next asked for. */
int32_t snesimage_reduce_characters(snesimage_ctx *ctx, uint32_t max_unique, uint32_t shortlist /*1..64, 0 = 16*/,
                                    snesimage_merge_result *log, uint32_t log_cap, uint32_t *merges, uint32_t *unique);
/* The tilemap of the image as it stands; conventions of snesimage_as_json (keys sorted, no spaces, the byte count returned):
 * "character": per tile, its class's position in "characters"; "characters": one 64-value array per class, classes ordered by
 * representative, in the representative's own orientation; "hflip", "vflip": per tile, 0 or 1, from flip_of; "palette": per
 * tile, tile_palettes.  Tile t is drawn as flip_f(characters[character[t]]), f = hflip[t] + 2 * vflip[t]. */
int64_t snesimage_as_tilemap_json(snesimage_ctx *ctx, char *out, int64_t cap);

/* The refit of shared characters — NOT a reference method.  A merge gives tile t the indices of a donor b: indices chosen for
 * b's pixels and b's subpalette.  A refit asks which 64 indices are best for ALL the tiles that share a character, each read
 * through its own subpalette and flip — the centroid update of vector quantisation.  Off unless called; no other entry point
 * changes.  Integers only, except the objective.  The terms are those of the character budget above; everything works on MAP
 * VALUES (in an unpinned tile a character value is the map value + 1, or 0 for the backdrop value of a backdrop context).
 * S is the context's internal subpalette size (sub_size + 1 in a backdrop context, whose backdrop B is entry S - 1 of every
 * subpalette).
 *   SNAPSHOT: at the start of a sweep, the classes of the stored map as it stands (an optimize() still owed runs first, as in
 *     snesimage_characters).  An ELIGIBLE CLASS has at least 2 members, none of them pinned.  Its members, its representative
 *     r = rep and the flips f_m = flip_of(m) are fixed for the whole sweep.  mask(f) = (f & 1 ? 7 : 0) | (f & 2 ? 56 : 0):
 *     member m's pixel q ^ mask(f_m) shows position q of the representative's orientation.
 *   FIT of an eligible class: for position q in 0..63 and value v in 0..S-1,
 *       cost(q, v) = sum over members m of red_mean_key(original pixel q ^ mask(f_m) of tile m,
 *                                                       8-bit expansion of entry tile_palettes[m] * S + v),
 *     the integer key of lib.rs:1080-1088 without the square root, summed in a uint64_t (below 2^39).  It reads the ORIGINAL
 *     image, never the ordered-dither target, and is this integer key whatever SNES_PERCEPTUAL says.  fitted[q] = the LOWEST v
 *     among the minima of cost(q, .); cur[q] = the representative's map value at q;
 *     gain = sum over q of cost(q, cur[q]) - cost(q, fitted[q]) >= 0.  The fit depends on the snapshot, the original and the
 *     palette only, not on the map: the fits of all classes of a sweep are computed once, up front.
 *   REFIT CALL on eligible class r: if fitted == cur the call is SKIPPED — not scored, changed = 0, the record's error is the
 *     incumbent.  Otherwise the candidate is the stored map with map(m; p) := fitted[p ^ mask(f_m)] for every member m and
 *     pixel p, nothing else changed; its error is error() of that stored map (no optimize(), no re-dither); acceptance is
 *     lib.rs:216-219: taken iff e < incumbent, strict.  Unlike a merge, which a constraint forces, a refit is an improvement:
 *     it is conditional and can never raise the error.
 *   REFIT SWEEP: the refit calls on the eligible classes in ascending rep order, each seeing the map and the incumbent the call
 *     before left (classes are disjoint tile sets: the candidates of later classes stay well defined after an acceptance).
 *     Afterwards, if anything was accepted, the state is that of snesimage_reduce_characters: a stored map with its error
 *     known, the epoch advanced.  A sweep that accepts nothing, or has no eligible class, leaves the context untouched bit
 *     for bit.  U never rises; it may fall if two classes become equal.  Like the reduction, A REFIT IS THE LAST STAGE OF A
 *     RUN: whatever re-runs optimize() replaces it.
 *   WINDOWS as snesimage_tile_sweep: a window builds and scores the candidates of the coming K non-skipped calls against the map
 *     as it stands in one launch group and commits them in order on the device up to the first that accepts; the calls behind
 *     it are scored again by the next window (one synchronisation per window).  window: 0 = chosen by the library, 1 = call by
 *     call, K = at most K calls per launch set (bounded by the launch group of the tile moves, at most 512).  For every window
 *     everything observable afterwards equals call by call, bit for bit.
 * Refusals: SNES_ERR_ARG for a null context, a rep beyond the image, a rep that is not the representative of an eligible class;
 * SNES_ERR_STATE between the phases of a split-phase step or window and on a context lent to a batch, a set or a group;
 * SNES_ERR_HIP after a failed workspace allocation, the context usable and unchanged. */
typedef struct { double error; uint64_t gain; uint16_t rep, members; uint8_t changed, scored; uint8_t pad[2]; } snesimage_refit_result; /* 24 bytes; error = the incumbent after the call */
/* The eligible classes of the image as it stands, ascending rep, with their fits: reps, members, gains hold up to ntile entries,
 * fits 64 map values per class in the representative's orientation; *n = classes.  Every array is optional.  State unchanged. */
int32_t snesimage_character_fits(snesimage_ctx *ctx, uint16_t *reps /*ntile*/, uint16_t *members /*ntile*/, uint64_t *gains /*ntile*/,
                                 uint8_t *fits /*ntile*64*/, uint32_t *n);
/* errors[j] of the refit candidates of n explicit classes (named by their representative, which must be eligible) against the
 * current state, which is left unchanged.  A class whose fit equals its character returns the incumbent error bit for bit.
 * maps_out (optional, n*w*h bytes): each candidate's palette_map.  Host pointers; synchronous; n may exceed the chunk. */
int32_t snesimage_score_refits(snesimage_ctx *ctx, const uint16_t *reps, uint32_t n, double *errors, uint8_t *maps_out /*opt, n*w*h*/);
/* One refit sweep.  log (optional): the first log_cap records in call order (skipped calls included, scored = 0); *calls = the
 * eligible classes; *accepted = calls taken; *unique = U afterwards; stats (optional) as snesimage_tile_sweep: calls, accepted,
 * windows, candidates scored, and `useful` = the scored calls that took effect.  If a window fails (SNES_ERR_HIP) the calls
 * accepted before it stand and are reported; the map is a stored map whose error is recomputed when next asked for. */
int32_t snesimage_refit_characters(snesimage_ctx *ctx, uint32_t window, snesimage_refit_result *log, uint32_t log_cap,
                                   uint32_t *calls, uint32_t *accepted, uint32_t *unique, snesimage_run_stats *stats);

/* The character budget of a shared-palette set — NOT a reference method.  On the console everything drawn on one background
 * reads one CGRAM, which the set models, and one VRAM character area: the two screens of a 512-wide level or the frames of an
 * animated background share one tileset.  These calls count and reduce the characters of ALL members together.  Everything is
 * an integer except the objective; the terms are those of the character budget above, extended as follows.
 *   GLOBAL TILE: a set of F members, each with ntile = 32 * h/8 tiles, has G = F * ntile global tiles, numbered
 *     g = member * ntile + tile (member-major).  The budget takes sets with G <= 8192 (eight frames of 256 x 256, nine of
 *     256 x 224); beyond that every call below answers SNES_ERR_UNSUPPORTED before touching anything.  The cap exists so that
 *     (cost, recipient, donor, flip) orders as one 64-bit key: a tile's cost is at most 64 * 299,505,150 < 2^35, which leaves
 *     13 bits each for recipient and donor.  The packing is internal; the order of the tuple is the contract.
 *   CHARACTER, FLIP, PINNED: unchanged, per tile, from its member's stored map and source alpha (sets refuse backdrop members:
 *     there is no backdrop value).
 *   SAME CHARACTER, rep(g), flip_of(g), U: as above but over all G tiles: rep(g) is the LOWEST GLOBAL INDEX of g's class, U the
 *     number of classes of the whole set.  A character that occurs in two members counts once.
 *   MERGE CANDIDATE (gt, gb, f), gt != gb, both unpinned: the recipient's member takes, in tile gt, the map values of tile gb
 *     — which may belong to ANOTHER member — under flip f.  The recipient keeps its own subpalette; nothing else changes, and
 *     no other member's map changes.  Its MEMBER ERROR e is error() of the recipient member's stored map with that tile
 *     rewritten (no optimize(), no re-dither).  Its INCREASE is d = e - inc_m, inc_m that member's incumbent error: one binary64
 *     subtraction; d may be negative.  Its PROXY COST is that of the single-image budget: the integer red-mean key summed over
 *     the recipient's 64 ORIGINAL pixels against the entries of the recipient's own subpalette that the donor's values name.
 *   ONE REDUCTION STEP with shortlist length K: recipients are the unpinned tiles ALONE in their set-wide class; a recipient's
 *     donors are the unpinned class representatives other than itself.  The shortlist is the K candidates lowest in
 *     (cost, gt, gb, f), fewer if fewer exist.  All are scored, each in its recipient's member.  The winner is the lowest
 *     (d, rank in the shortlist) — members' errors differ in size, their increases compare — a NaN never wins; it is applied
 *     UNCONDITIONALLY.  Afterwards the recipient member's map is the candidate's and its incumbent the candidate's scored bits;
 *     E is the members' incumbents summed in member order, as snesimage_shared_error sums; U has fallen by exactly one.
 *   REDUCTION to max_unique: steps while U > max_unique and a pair exists.  Running out of pairs is no error.
 *   STATE AFTERWARDS: every member that received a merge is as after snesimage_reduce_characters — a stored map, its error
 *     known, its epoch advanced — and the set records the new epochs: it stays intact.  snesimage_shared_error returns the last
 *     record's `error` bit for bit; the members' as_json, get_palette_map and as_rgba read the merged maps.  REDUCTION IS THE
 *     LAST STAGE OF A RUN: every set call that optimizes — snesimage_shared_step*, _run_slots, _slots_reserve, _tile_sweep,
 *     _reassign_tiles, the initialisers and the palette setter — first re-runs optimize() on every member that holds a merged
 *     map and then behaves exactly as on a set that never reduced.  snesimage_shared_error, _score_candidates and the calls
 *     below leave the merged maps.  A budget already met takes no step and leaves set and members untouched bit for bit.
 * Refusals mirror the single-image calls: SNES_ERR_ARG for null pointers, a member or tile out of range, a pinned tile named,
 * gt == gb, f > 3, max_unique == 0, shortlist > 64; SNES_ERR_STATE as every set call (a member changed outside the set, or a
 * member destroyed: that is answered before any member is read); SNES_ERR_HIP after a failed workspace allocation, set and
 * members usable and unchanged.  If a step fails the steps before it stand and are reported; the members that had a
 * candidate in it hold "a stored map of unknown error". */
typedef struct { double error, member_error; uint64_t cost; uint16_t member, tile, donor_member, donor, unique;
                 uint8_t flip, rank; uint8_t pad[4]; } snesimage_shared_merge_result; /* 40 bytes; error = E after the step, member_error = e, unique = U after it */
/* U, and optionally rep (G, global indices), flip_of (G) and the characters (G * 64) of the set as it stands. */
int32_t snesimage_shared_characters(snesimage_shared *set, uint32_t *unique, uint16_t *rep /*G, global, opt*/, uint8_t *flip /*G, opt*/,
                                    uint8_t *chars /*G*64, opt*/);
/* The shortlist a reduction step with length k (1..64, 0 = 16) would score, in rank order; *n = min(k, candidates that exist).
 * Output arrays (each optional) hold k entries: recipient (member, tile), donor (member, tile), flip, proxy cost.  State unchanged. */
int32_t snesimage_shared_merge_shortlist(snesimage_shared *set, uint32_t k, uint16_t *members, uint16_t *tiles, uint16_t *donor_members,
                                         uint16_t *donors, uint8_t *flips, uint64_t *costs, uint32_t *n);
/* errors[j] = the member error e of n explicit candidates — any unpinned pair — against the current state, which is left
 * unchanged.  A candidate that changes nothing returns its member's incumbent bit for bit.  maps_out (optional, n*w*h bytes):
 * each candidate's palette_map of the recipient's member.  Host pointers; synchronous. */
int32_t snesimage_shared_score_merges(snesimage_shared *set, const uint16_t *members, const uint16_t *tiles, const uint16_t *donor_members,
                                      const uint16_t *donors, const uint8_t *flips, uint32_t n, double *errors /*e: the recipient member's*/,
                                      uint8_t *maps_out /*opt, n*w*h*/);
/* The reduction.  log (optional): the first log_cap steps' records; *merges: steps taken; *unique: U afterwards. */
int32_t snesimage_shared_reduce_characters(snesimage_shared *set, uint32_t max_unique, uint32_t shortlist /*1..64, 0 = 16*/,
                                           snesimage_shared_merge_result *log, uint32_t log_cap, uint32_t *merges, uint32_t *unique);
/* The tilemap of the set as it stands, conventions of snesimage_as_tilemap_json: "characters" is ONE list for the whole set,
 * classes ordered by representative, each in the representative's orientation; "character", "hflip", "palette" and "vflip" are
 * lists of F lists, in member order. */
int64_t snesimage_shared_as_tilemap_json(snesimage_shared *set, char *out, int64_t cap);

/* Native export — NOT a reference method.  The result as the console loads it: a CGRAM image, bitplane character data (CHR) and
 * tilemap words (MAP), and a renderer that reads such bytes back as the PPU's background fetch does.  Off unless called; no other
 * entry point changes.  Terms are those of the character budget above: CHARACTER, FLIP, rep, flip_of, U, classes ordered by
 * representative.  S is the user's sub_size (in a backdrop context the user's size, not the expanded one), C is sub_count.
 *   DEPTH: bpp = 0 picks the smallest of 2 (S <= 3), 4 (S <= 15) and 8.  An explicit depth must hold S, S <= (1 << bpp) - 1, else
 *     SNES_ERR_ARG.  8bpp requires C == 1 and palette_base == 0 — the 8bpp tilemap word's palette bits do not select among
 *     256-colour palettes — else SNES_ERR_UNSUPPORTED, the message names the geometry.  2bpp and 4bpp require
 *     palette_base + C <= 8, else SNES_ERR_ARG.
 *   CGRAM: 512 bytes, 256 little-endian words r | g << 5 | b << 10, the words snesimage_get_palette_u16 returns.  Row p starts at
 *     word (palette_base + p) << bpp for 2bpp and 4bpp and at word 0 for 8bpp; entry i of row p sits at the row's start + 1 + i.
 *     The word at each row's start, and word 0 of CGRAM, hold B in a backdrop context and 0 otherwise — what snesimage_as_json
 *     writes into slot 0 of every row.  Every other word is 0.  At 4bpp with palette_base 0 CGRAM is therefore the JSON's
 *     `palette` rows concatenated and zero-padded.
 *   CHR: U characters in class order — the order of "characters" in the tilemap JSON — each in its representative's orientation,
 *     8 * bpp bytes.  For plane pair k (planes 2k and 2k + 1) and row y, byte 16k + 2y is plane 2k of row y and byte 16k + 2y + 1
 *     plane 2k + 1; bit 7 - x of a plane byte is that plane's bit of the character value at (x, y).  The values are the
 *     CHARACTER values (0 for a transparent or backdrop pixel, map + 1 otherwise); the depth condition makes them fit.
 *   MAP: ntile little-endian words in tile order t = ty * 32 + tx — the picture is 32 tiles wide, so this is the top h/8 rows
 *     of one 32 x 32 screen.  word = (char_base + pos(rep(t))) | (palette_base + tile_palettes[t]) << 10 | priority << 13 |
 *     hflip << 14 | vflip << 15, pos(r) the position of r's class in CHR, hflip and vflip bits 0 and 1 of flip_of(t); the
 *     palette field is 0 at 8bpp.  char_base + U <= 1024 is required, else SNES_ERR_ARG with a message that states U and names
 *     the character budget calls.
 * snesimage_export_native produces all three pieces from one state; every output is optional, a call with none only fills
 * `info`.  chr_cap < chr_bytes with chr given is SNES_ERR_ARG.  It works as snesimage_characters does (an optimize() still owed
 * is run first) and leaves the state unchanged bit for bit: map, error, epoch.  Refusals are those of snesimage_characters plus
 * the ones above; a refusal leaves the context usable.
 * snesimage_shared_export_native counts classes over all members (global representative order: ONE CHR for the set) and writes
 * one map per member, member-major.  A backdrop set answers SNES_ERR_UNSUPPORTED as snesimage_shared_as_tilemap_json does, more
 * than 8,192 tiles in all as the set's character calls do.
 * snesimage_render_native decodes cgram, chr and map under the same layout into w*h RGBA: per pixel the tilemap word, the flips,
 * the plane bytes, the index; index 0 reads CGRAM word 0, any other the row's start + index (8bpp: the index itself); 5 -> 8 bits
 * as v * 8 + v / 4; alpha 255.  It reads the context's width, height, device and stream and nothing of its palette or map (bpp = 0
 * resolves from the context's S), so it judges bytes from anywhere, on a lent context too.  Inputs are checked before any
 * launch: a null pointer, chr_bytes that is not 1..1024 whole characters, or a map word whose character number lies below
 * char_base or beyond chr_bytes is SNES_ERR_ARG.
 * Out of scope: backdrop sets, 8bpp with several subpalettes, widths other than 256, more than one 32 x 32 screen and compression.
 * Native files are read back by the native import below. */
typedef struct { uint8_t bpp /*0 = auto, 2, 4, 8*/, palette_base /*0..7*/, priority /*0, 1*/, pad; uint16_t char_base /*0..1023*/, pad2; } snesimage_native_layout; /* 8 bytes; NULL = all zero */
typedef struct { uint32_t bpp, unique, chr_bytes, map_words; } snesimage_native_info;
int32_t snesimage_export_native(snesimage_ctx *ctx, const snesimage_native_layout *layout, uint8_t *cgram /*512, opt*/, uint8_t *chr /*opt*/, uint64_t chr_cap,
                                uint16_t *map /*ntile, opt*/, snesimage_native_info *info /*opt*/);
int32_t snesimage_shared_export_native(snesimage_shared *set, const snesimage_native_layout *layout, uint8_t *cgram, uint8_t *chr, uint64_t chr_cap,
                                       uint16_t *maps /*F * ntile, member-major, opt*/, snesimage_native_info *info);
int32_t snesimage_render_native(snesimage_ctx *ctx, const snesimage_native_layout *layout, const uint8_t *cgram /*512*/, const uint8_t *chr, uint64_t chr_bytes,
                                const uint16_t *map /*ntile*/, uint8_t *rgba /*w*h*4*/);

/* Native import — NOT a reference method.  The inverse of the native export: CGRAM, CHR and MAP bytes — the export's own, or
 * bytes ripped from a ROM or drawn in a tile editor — decoded into the STATE of a context of the same picture: palette, backdrop
 * colour, tile_palettes and a stored palette_map.  Off unless called; no other entry point changes.  The terms are the export's:
 * S is the user's sub_size, C is sub_count, and `layout` is resolved and refused exactly as the export resolves and refuses it
 * for (S, C): the depth (0 = the smallest that holds S), S <= (1 << bpp) - 1, 8bpp only with C == 1 and palette_base 0,
 * palette_base + C <= 8.  `priority` is not read.  chr_bytes must be 1..1024 whole cells of 8 * bpp bytes, else SNES_ERR_ARG.
 *   PER TILE t, with the word w = map[t]:
 *     the character number n = w & 1023 must satisfy char_base <= n < char_base + chr_bytes / (8 * bpp);
 *     the palette field p = (w >> 10) & 7: at 2bpp and 4bpp tile_palettes[t] = p - palette_base, which must lie in 0..C-1; at 8bpp
 *     the field is ignored and the subpalette is 0;
 *     the priority bit (13) is ignored; bits 14 and 15 are the horizontal and the vertical flip.
 *   PER PIXEL (x, y) of tile t the value v is decoded exactly as snesimage_render_native decodes it: the flips first (cell column
 *     7 - x under hflip, cell row 7 - y under vflip), then the plane bytes of cell n - char_base in the export's CHR layout.
 *       v >= 1: the map value is v - 1, which must be < S;
 *       v == 0 where the source alpha is 0: accepted; the stored map value there is 0, and nothing observable reads it (as_json,
 *         as_rgba, the characters and error() treat such a pixel as transparent);
 *       v == 0 where the source alpha is not 0: in a SNES_BACKDROP context the map value S (the tied entry: the backdrop colour
 *         shows); in any other context refused — the message says to create the context with SNES_BACKDROP;
 *       v != 0 where the source alpha is 0: refused; the library has no way to draw it.
 *   CGRAM: entry i of row p is word ((palette_base + p) << bpp) + 1 + i (8bpp: word 1 + i) as raw 5-bit r, g, b; bit 15 is
 *     dropped.  A backdrop context takes B from word 0 and only from word 0: the rows' first words are not read, as the hardware
 *     does not read them for a background.  Words the geometry does not name are not read either: foreign files need not be zero
 *     there.  On a SNES_NES context the colours are taken as they are, not snapped to the NES table; the setters do the same.
 *   DUPLICATES: duplicate, unused and differently ordered cells are all fine.  The import is per tile.
 *   ALL OR NOTHING: everything is decoded into staging buffers on the context's stream and a verdict read back after one
 *     synchronisation; only then are palette, tile_palettes (entries [0, ntile); the rest of the 1,024 stay) and map copied into
 *     the context.  A refusal under PER TILE or PER PIXEL is SNES_ERR_ARG; its message names the LOWEST offending tile and that
 *     tile's reason (of several reasons in one tile the first in the order: number below char_base, number past the cells,
 *     palette field, value above S, 0 on an opaque pixel, colour on a transparent pixel; a tile whose number is refused is not
 *     decoded further).  A refusal leaves palette, tile_palettes, map, incumbent error, epoch and a pending optimize() exactly as
 *     they were.
 *   STATE AFTERWARDS: as after snesimage_set_palette_rgb5, snesimage_set_backdrop_rgb5, snesimage_set_tile_palettes and
 *     snesimage_set_palette_map with the decoded values, in one step: a stored map whose error is unknown; a pending optimize()
 *     is dropped, as snesimage_set_palette_map drops it; tables, packs and the incumbent are invalid and the epoch has advanced.
 *     Whatever re-runs optimize() replaces the map, as with any stored map; the character budget, the refit, the tilemap, the
 *     export and snesimage_error read it as it stands.  An ordered-dither table or level bank stays set.
 * Refusals beyond those above are those of snesimage_characters (a null context, between the phases of a split-phase step or
 * window, a context lent to a batch, a set or a group) and null pointers.  info (optional): bpp, unique = the number of cells in
 * chr, chr_bytes and map_words.
 * snesimage_shared_import_native does the same for a set: ONE palette, written to every member; each member's tile_palettes and
 * stored map come from its slice of `maps` (member-major, as snesimage_shared_export_native writes them); the lowest offending
 * tile is the lowest GLOBAL tile and the message names its member.  All or nothing over the whole set: one verdict for all
 * members before any member is touched.  Afterwards the set is as an accepted snesimage_shared_reduce_characters leaves it: the
 * members carry stored maps, the set has recorded their epochs and stays intact, and it remembers that it holds merged maps, so
 * every set call that optimizes re-runs optimize() first; E is unknown until snesimage_shared_error.  A backdrop set answers
 * SNES_ERR_UNSUPPORTED as snesimage_shared_export_native does, a retired set or a member changed outside SNES_ERR_STATE, more than
 * 8,192 tiles in all SNES_ERR_UNSUPPORTED as the set's character calls do.
 * Out of scope: backdrop sets, widths other than 256, more than one 32 x 32 screen, compression. */
int32_t snesimage_import_native(snesimage_ctx *ctx, const snesimage_native_layout *layout, const uint8_t *cgram /*512*/, const uint8_t *chr, uint64_t chr_bytes,
                                const uint16_t *map /*ntile*/, snesimage_native_info *info /*opt*/);
int32_t snesimage_shared_import_native(snesimage_shared *set, const snesimage_native_layout *layout, const uint8_t *cgram /*512*/, const uint8_t *chr, uint64_t chr_bytes,
                                       const uint16_t *maps /*F * ntile, member-major*/, snesimage_native_info *info /*opt*/);

/* The refit of shared characters across the members of a shared-palette set — NOT a reference method.  After a set merge a
 * character that serves tiles of several frames still carries the indices chosen for one donor tile of one frame.  This is the
 * refit above over the whole set: each shared character fitted to ALL the tiles of ALL members that use it, decided on the joint
 * error.  Off unless called; no other entry point changes.  The terms are those of "the refit of shared characters" and of "the
 * character budget of a shared-palette set" (global tile g = member * ntile + tile; sets hold no backdrop member, so a map value
 * is a character value - 1 in every unpinned tile; S is the subpalette size).
 *   SNAPSHOT: at the start of a sweep, the SET-WIDE classes of the members' stored maps as they stand: rep(g) is the lowest
 *     GLOBAL tile of g's class, flip_of(g) as defined.  An optimize() still owed runs first, as in snesimage_shared_characters;
 *     merged maps stay.  An ELIGIBLE CLASS has at least 2 global tiles, none of them pinned (in whichever member).  Its tiles, its
 *     representative r and the flips f_g are fixed for the whole sweep.  Its TOUCHED MEMBERS are the members that hold at least
 *     one of its tiles.
 *   FIT of an eligible class: for position q in 0..63 and value v in 0..S-1,
 *       cost(q, v) = sum over the class's global tiles g = (m, t) of red_mean_key(original pixel q ^ mask(f_g) of tile t of
 *                                member m, 8-bit expansion of entry tile_palettes_m[t] * S + v of the shared palette),
 *     summed in a uint64_t: at most 8,192 terms of at most 299,505,150 each, so below 2^42, and cost << 8 | v still fits.
 *     fitted[q] = the LOWEST v among the minima of cost(q, .); cur[q] = the representative's map value at q;
 *     gain = sum over q of cost(q, cur[q]) - cost(q, fitted[q]) >= 0.  The fit reads the members' ORIGINALS, never an
 *     ordered-dither target, and is this integer key whatever SNES_PERCEPTUAL says.  It depends on the snapshot, the originals
 *     and the palette only: the fits of all classes of a sweep are computed once, up front.
 *   REFIT CALL on eligible class r: if fitted == cur the call is SKIPPED — not scored, changed = 0, the record's error is E.
 *     Otherwise the candidate gives every tile g of the class map(g; p) := fitted[p ^ mask(f_g)] in its own member's stored map;
 *     nothing else changes.  For each touched member i, e_i is error() of that member's candidate map (no optimize(), no
 *     re-dither).  With inc_i the members' incumbent errors, E' = sum over i of (e_i if i is touched, else inc_i) and
 *     E = sum over i of inc_i, both summed in member order, left to right, with plain + (as snesimage_shared_error sums).  The
 *     candidate is taken iff E' < E, strict (lib.rs:216-219 applied to the joint error, as every set call decides); a NaN in
 *     any e_i never wins.  On acceptance every touched member takes its candidate map and e_i as its incumbent.  A SINGLE
 *     MEMBER'S ERROR MAY RISE as long as E falls: the set is one picture budget, and the decision is the set's.
 *   REFIT SWEEP: the calls on the eligible classes in ascending global rep, each seeing the maps and the incumbents the call
 *     before left (classes are disjoint sets of tiles).  U never rises; it may fall if two classes become equal.
 *   WINDOWS as snesimage_refit_characters: a window builds and scores the candidates of the coming K non-skipped calls against
 *     the maps as they stand — each touched member scores its share in its own tile workspace — and one commit walks the calls
 *     in order up to the first that accepts; the calls behind it are scored again by the next window.  One synchronisation per
 *     window.  window: 0 = chosen by the library, 1 = call by call, K = at most K calls per launch set (bounded by the launch
 *     group of the tile moves and by 64, a member's share of a set's launch set).  For every window the records, maps,
 *     incumbents and epochs afterwards are the same, bit for bit.
 *   STATE AFTERWARDS: if a call was accepted, that of snesimage_shared_reduce_characters: every member touched by an accepted
 *     call holds a stored map with its error known and its epoch advanced, the set records the new epochs and stays intact,
 *     snesimage_shared_error returns the last accepted E bit for bit, and the set remembers that it holds merged maps: every set
 *     call that optimizes re-runs optimize() first.  A REFIT IS THE LAST STAGE OF A RUN.  A sweep that accepts nothing — no
 *     eligible class, only skipped calls, or every scored call rejected — leaves the set and every member untouched bit for
 *     bit.  Between enqueuing a window's commit and reading its records every member touched by a call of that window is flagged
 *     "a stored map of unknown error"; the members that no accepted call touched get their flags and epoch back, as in the set's
 *     merge step.  If a window fails (SNES_ERR_HIP) the calls accepted before it stand and are reported.
 * Refusals mirror the two blocks this extends: SNES_ERR_ARG for null pointers, a rep beyond G, a rep that does not represent an
 * eligible class; SNES_ERR_UNSUPPORTED for G > 8,192, before anything is touched; SNES_ERR_STATE as every set call;
 * SNES_ERR_HIP after a failed workspace allocation, set and members usable and unchanged. */
typedef struct { double error; uint64_t gain; uint16_t rep, members, touched; uint8_t changed, scored; } snesimage_shared_refit_result; /* 24 bytes; error = E after the call; rep global; members = the class's tiles; touched = its members */
/* The eligible classes of the set as it stands, ascending global rep, with their fits: reps, members (tiles in the class), gains
 * hold up to G entries, fits 64 map values per class in the representative's orientation; *n = classes.  Every array is
 * optional.  State unchanged. */
int32_t snesimage_shared_character_fits(snesimage_shared *set, uint16_t *reps /*G, global*/, uint16_t *members /*G*/, uint64_t *gains /*G*/,
                                        uint8_t *fits /*G*64*/, uint32_t *n);
/* errors[j] = E' of the refit candidate of class reps[j] (global representatives, each eligible) against the current state,
 * which is left unchanged.  member_errors (optional, n*F): e_i, or inc_i bit for bit for an untouched member.  maps_out
 * (optional, n*F*w*h bytes): every member's candidate map, the stored map for an untouched member.  A class whose fit equals its
 * character returns E bit for bit.  Host pointers; synchronous; n may exceed a launch group. */
int32_t snesimage_shared_score_refits(snesimage_shared *set, const uint16_t *reps, uint32_t n, double *errors /*E' per class*/,
                                      double *member_errors /*opt, n*F*/, uint8_t *maps_out /*opt, n*F*w*h*/);
/* One refit sweep.  log (optional): the first log_cap records in call order (skipped calls included, scored = 0); *calls = the
 * eligible classes; *accepted = calls taken; *unique = U afterwards; stats (optional) as snesimage_refit_characters. */
int32_t snesimage_shared_refit_characters(snesimage_shared *set, uint32_t window, snesimage_shared_refit_result *log, uint32_t log_cap,
                                          uint32_t *calls, uint32_t *accepted, uint32_t *unique, snesimage_run_stats *stats);

/* State access (the reference mutates these fields directly: lib.rs:1015 and the GUI). */
int32_t snesimage_get_tile_palettes(snesimage_ctx *ctx, uint8_t *out /*1024*/);
int32_t snesimage_set_tile_palettes(snesimage_ctx *ctx, const uint8_t *in /*1024*/);
int32_t snesimage_get_palette_rgb5(snesimage_ctx *ctx, uint8_t *out /*count*size*3*/);
int32_t snesimage_set_palette_rgb5(snesimage_ctx *ctx, const uint8_t *in);
int32_t snesimage_get_palette_u16(snesimage_ctx *ctx, uint16_t *out /*count*size; lib.rs:679-681*/);
/* The backdrop colour B of a backdrop context (SNES_ERR_ARG on any other), raw 5-bit r,g,b.  Setting it invalidates
 * palette_map as snesimage_set_palette_rgb5 does: call snesimage_optimize() before reading the map or the error. */
int32_t snesimage_get_backdrop_rgb5(snesimage_ctx *ctx, uint8_t *out /*3*/);
int32_t snesimage_set_backdrop_rgb5(snesimage_ctx *ctx, const uint8_t *in /*3*/);
/* NOT a reference mode: ordered dithering.  The reference's only dithering is Floyd-Steinberg error diffusion (SNES_DITHER,
 * lib.rs:425-501): a serial pass per candidate, and unstable from frame to frame.  An ORDERED-DITHER TABLE is n*n offsets
 * (n = 2, 4, 8 or 16; int8_t, row-major, indexed [y % n][x % n]; any values: a Bayer matrix, a blue-noise tile) added to the
 * picture before the nearest-colour choice.  With a table set the context keeps a TARGET IMAGE T beside the original:
 * T.c = clamp(orig.c + d[y % n][x % n], 0, 255) for c = r, g, b (one offset for the three channels), T.a = orig.a — the
 * clamp of lib.rs:773-778 on an integer.  Everything in integers, so every result stays bit-exact.
 *   - T replaces the original wherever the nearest-colour choice of lib.rs:762-795 is made: snesimage_optimize(), the
 *     candidates' remap in snesimage_score_candidates(_device), snesimage_remap_candidates_device, the steps, windows, batches,
 *     sets and groups, the costs of snesimage_reassign_tiles and the tile moves; with SNES_PERCEPTUAL the distances are taken
 *     from Lab(T);
 *   - the original stays what error() compares with (lib.rs:503-548: the optimizer sees the dithering when it scores a
 *     palette, TODO.md:21-26), what both k-means initialisers cluster (their closing optimize() sees T), what the backdrop's
 *     initial mean is taken from, and what as_rgba's alpha and the JSON's transparency rule read;
 *   - a pixel's target depends on no other pixel: a context with a table takes every path of a context without SNES_DITHER
 *     (the group-sparse scorer, slot windows, duplicate sharing, batches, sets, groups, tile moves, the backdrop: B is one
 *     more entry in the choice against T);
 *   - without a table T is the original itself (the same buffer) and the context issues exactly the launches it always did;
 *     an all-zero table gives T == orig value for value.
 * snesimage_set_ordered_dither: n = 0 (offsets may be NULL) switches the table off.  It invalidates what
 * snesimage_set_palette_rgb5 invalidates — call snesimage_optimize() before reading the map or the error — and what the slot
 * windows and the tile moves keep per image; the source side of error() stays valid.  Refusals: SNES_ERR_ARG for a null
 * context, n outside {0, 2, 4, 8, 16} or a null table with n > 0; SNES_ERR_UNSUPPORTED for n > 0 on a SNES_DITHER context (the
 * two are alternatives); SNES_ERR_STATE between the phases of a split-phase step or window and on a context lent to a batch,
 * group or set.  snesimage_batch_create, snesimage_group_create and snesimage_shared_create refuse members whose tables
 * differ (SNES_ERR_ARG), as they refuse differing flags.  The JSON does not record the table.
 * snesimage_get_ordered_dither: the table (256 bytes, zeros behind the n*n offsets) and *n (0: none).
 * snesimage_get_target_rgba: T as w*h*4 bytes (the original while no table is set).
 * snesimage_bayer_offsets (host helper): the Bayer table of side n and amplitude A in 1..255 — M_1 = [0],
 * M_2n = [[4M, 4M+2], [4M+3, 4M+1]]; num = A*(2*M + 1 - n*n), den = 2*n*n, d = sign(num) * ((2*|num| + den) / (2*den)) in
 * integer division: A*((M + 1/2)/(n*n) - 1/2) rounded half away from zero.  Every such table sums to 0; (2, 64) is
 * [-24, 8, 24, -8].  Any other n or A writes nothing. */
int32_t snesimage_set_ordered_dither(snesimage_ctx *ctx, const int8_t *offsets /* n*n */, uint32_t n);
int32_t snesimage_get_ordered_dither(snesimage_ctx *ctx, int8_t *out /* 256 */, uint32_t *n);
int32_t snesimage_get_target_rgba(snesimage_ctx *ctx, uint8_t *out /* w*h*4: T */);
void    snesimage_bayer_offsets(uint32_t n, uint32_t amplitude, int8_t *out /* n*n */);
/* NOT a reference method: per-tile ordered-dither LEVELS, chosen by the objective (DESIGN 5d').  Gradients want the full
 * amplitude; flat areas, outlines and text look worse with any.  A BANK is L tables (1 <= L <= 8) of one side n (2, 4, 8 or 16;
 * int8_t, row-major, any values; an all-zero table means "no dithering"), and every tile t = ty*32 + tx is on one of them:
 * level[t] in [0, L).  The target image becomes T.c(x, y) = clamp(orig.c + bank[level[tile(x, y)]][y % n][x % n], 0, 255),
 * T.a = orig.a.  The pattern's phase stays in image coordinates: neighbouring tiles on one level join seamlessly, and a 16 x 16
 * table spans two tiles.  With L = 1 this is the T of snesimage_set_ordered_dither, and everything said there about who reads T
 * holds for any L: no existing entry point changes.
 *   A LEVEL CALL on tile t with cur = level[t]: for l = 0 .. L-1 ascending, l != cur, e_l = error() of the state with
 * level[t] := l and optimize() run (palette and tile_palettes untouched: the map differs from the current one in the tile's
 * 64 pixels at most); acceptance as lib.rs:216-219 — best := incumbent, a strict e_l < best is taken.  If one was taken the
 * state becomes that candidate's (level[t], T on that tile, palette_map, the incumbent error), otherwise it is untouched bit
 * for bit.  A level whose 64 choices equal the current ones gives e_l == incumbent exactly and is never taken.
 *   A LEVEL SWEEP is the level calls on first_tile .. first_tile + n_tiles - 1 in order, each seeing the state the one before
 * left, run in windows exactly as snesimage_tile_sweep runs them (window 0: chosen by the library; 1: call by call; K: at most
 * K calls per launch set; one synchronisation per window); every window size gives everything observable bit for bit equal to
 * call by call.  The record's `sub` field carries the tile's level after the call.  After an accepted call the context is as
 * snesimage_set_tile_levels + snesimage_optimize would leave it, with the incumbent error known.  A window that fails leaves
 * the accepted calls standing and reported.
 * snesimage_set_ordered_dither_bank: sets the bank, every tile on start_level.  It invalidates what
 * snesimage_set_ordered_dither invalidates and has its refusals (SNES_ERR_UNSUPPORTED on a SNES_DITHER context, SNES_ERR_STATE
 * between the phases of a split-phase step or on a lent context; SNES_ERR_ARG for n outside {0, 2, 4, 8, 16}, L > 8, a null
 * bank or start_level >= L).  L = 0 or n = 0 switches ordered dithering off.
 * snesimage_get_ordered_dither_bank: 8 * 256 bytes, table l at 256 * l (zeros behind the n*n offsets), *n and *L (0: none).
 * snesimage_get_tile_levels / snesimage_set_tile_levels: 1024 bytes as snesimage_get_tile_palettes (0 for the rows of tiles
 * below the image, whatever is set there); a value >= L on a tile of the image is SNES_ERR_ARG, no bank SNES_ERR_STATE; invalidation and refusals as for the bank setter.
 * snesimage_score_tile_levels: e_j of explicit (tile, level) pairs, the state left unchanged; a pair naming the tile's current
 * level returns the incumbent bit for bit; n may exceed the chunk (launch groups as in snesimage_score_tile_moves); maps_out
 * (optional): n palette_maps of w*h bytes.
 * On a context with L > 1: snesimage_set_ordered_dither replaces the bank by a bank of one; snesimage_get_ordered_dither
 * answers SNES_ERR_STATE (use the bank getter); snesimage_batch_create, snesimage_shared_create and snesimage_group_create
 * refuse the member with SNES_ERR_ARG — sets and groups share launches and one table. */
int32_t snesimage_set_ordered_dither_bank(snesimage_ctx *ctx, const int8_t *tables /* L*n*n */, uint32_t n, uint32_t L, uint32_t start_level);
int32_t snesimage_get_ordered_dither_bank(snesimage_ctx *ctx, int8_t *tables /* 8*256 */, uint32_t *n, uint32_t *L);
int32_t snesimage_get_tile_levels(snesimage_ctx *ctx, uint8_t *out /* 1024 */);
int32_t snesimage_set_tile_levels(snesimage_ctx *ctx, const uint8_t *in /* 1024 */);
int32_t snesimage_score_tile_levels(snesimage_ctx *ctx, const uint16_t *tiles, const uint8_t *levels, uint32_t n, double *errors, uint8_t *maps_out /* optional */);
int32_t snesimage_level_step(snesimage_ctx *ctx, uint32_t tile, snesimage_tile_result *out);
int32_t snesimage_level_sweep(snesimage_ctx *ctx, uint32_t first_tile, uint32_t n_tiles, uint32_t window, snesimage_tile_result *log, snesimage_run_stats *stats);
/* NOT a reference method: per-tile ordered-dither levels on a SHARED-PALETTE SET, tied or per frame (DESIGN 5d'').  The
 * refusals above stand — snesimage_shared_create takes no member with L > 1, and a lent member's own setters answer
 * SNES_ERR_STATE — so a set gets its bank through the set: the SET owns the bank, every member holds it and a level per tile of
 * its own, and reads its own T.  F = the number of members; E = the members' error() summed in member order, first then plain +,
 * as snesimage_shared_error sums.  A level chosen frame by frame makes a static tile's pattern switch on and off between
 * frames, the shimmer ordered dithering is there to remove; hence the TIED level: one level per tile position for all frames.
 *   A TIED LEVEL CALL on tile position t, every member's level[t] being the common cur: for l = 0 .. L-1 ascending, l != cur,
 * E_l = the sum in member order of e_{m,l}, e_{m,l} = error() of member m with level_m[t] := l and optimize() run (a member whose
 * 64 choices do not change gives its incumbent exactly); acceptance as lib.rs:216-219 on E — best := E, a strict E_l < best is
 * taken.  An accepted call changes level[t], tile t of T (and of Lab(T)), the palette_map and the incumbent error in EVERY member,
 * members whose map does not change and members whose own error rises included; otherwise every member is untouched bit for bit.
 *   A TIED LEVEL SWEEP is the tied calls on first_tile .. first_tile + n_tiles - 1 in order, each seeing the state the one
 * before left, run in windows (window 0: chosen by the library; 1: call by call; K: at most K calls per launch set; one
 * synchronisation per window; a member's share of a window is at most its launch group, see snesimage_score_tile_moves); every
 * window size gives everything observable bit for bit equal to call by call.  A window that accepts nothing leaves every member
 * untouched bit for bit; a window that fails leaves the accepted calls standing and reported.
 * snesimage_shared_set_ordered_dither_bank: arguments and their validation as snesimage_set_ordered_dither_bank (SNES_ERR_ARG
 * for a null set, n outside {0, 2, 4, 8, 16}, L > 8, a null bank, start_level >= L); the bank goes to every member with every
 * tile of every member on start_level; L = 0 or n = 0 switches the tables of all members off.  SNES_ERR_UNSUPPORTED for a set of
 * SNES_DITHER members, SNES_ERR_STATE while a split-phase step or window of a member is pending.  A failed allocation
 * (SNES_ERR_HIP) leaves every member as it was: T, bank and levels.  Afterwards the set is settled as after
 * snesimage_shared_set_palette_rgb5: optimize() has run on every member and the incumbents are known.  After
 * snesimage_shared_destroy the members keep bank and levels, as lone contexts with a bank do.
 * snesimage_shared_set_tile_levels: snesimage_set_tile_levels on member `member` (1024 bytes; a value >= L on a tile of the
 * image or member >= F is SNES_ERR_ARG, no bank SNES_ERR_STATE), the set settled afterwards; snesimage_get_tile_levels on the
 * member reads the levels back.
 * snesimage_shared_score_tile_levels: pair j is "every member's tile tiles[j] on levels[j]"; member_errors[j*F + m] (optional)
 * is member m's error — its incumbent, bit for bit, where its tile is on that level already or its 64 choices do not change —
 * and errors[j] their sum in member order.  The state is left unchanged; n may exceed the chunk.  SNES_ERR_ARG for a tile beyond
 * the image or a level beyond the bank; SNES_ERR_STATE without a bank, and on a set whose stored maps are a character
 * reduction's (no optimize() of the palette: the call does not replace them).
 * snesimage_shared_level_sweep: tied != 0: the tied level sweep; log holds n_tiles records (error = E after the call, sub = the
 * common level after it, changed); SNES_ERR_STATE, before any work, when the members differ in level on a tile of the range.
 * tied == 0: snesimage_level_sweep on every member, member after member, each call decided on the member's own error as
 * snesimage_shared_tile_sweep decides; log holds F * n_tiles records, member-major.  Both: window and stats as for
 * snesimage_level_sweep (stats summed over the members; a tied window scores each of its candidates F times); SNES_ERR_ARG for
 * a tile range beyond the image, SNES_ERR_STATE without a bank; like every set call that optimizes, the sweep first replaces the
 * merged maps of an earlier character reduction by optimize().  With a bank of one table nothing is scored or accepted. */
int32_t snesimage_shared_set_ordered_dither_bank(snesimage_shared *set, const int8_t *tables /* L*n*n */, uint32_t n, uint32_t L, uint32_t start_level);
int32_t snesimage_shared_set_tile_levels(snesimage_shared *set, uint32_t member, const uint8_t *levels /* 1024 */);
int32_t snesimage_shared_score_tile_levels(snesimage_shared *set, const uint16_t *tiles, const uint8_t *levels, uint32_t n, double *errors, double *member_errors /* n*F, optional */);
int32_t snesimage_shared_level_sweep(snesimage_shared *set, uint32_t first_tile, uint32_t n_tiles, uint32_t window, uint32_t tied, snesimage_tile_result *log, snesimage_run_stats *stats);
/* NOT a reference method: GUIDED CALLS.  optimize_palette_entry_random (lib.rs:191-240) draws its candidates
 * uniformly from the 32,768 colours of BGR555; the reference's TODO.md:33-35 asks for something better.  A guided call ranks
 * ALL 32,768 colours for the slot by a cheap, exact, integer proxy and lets error() decide among the K the proxy likes, as the
 * merges of the character budget do.  Off unless called: no other entry point changes, snesimage_step keeps refusing
 * method > 2.  Integers only, except the objective.  For a slot (p, i) of a context (C, S):
 *   POPULATION: the pixels with alpha > 0 in tiles with tile_palettes[t] == p.  Colours are those of the TARGET image T (the
 *     original, or what an ordered-dither table or bank made of it).
 *   FLOOR m(x): the minimum of red_mean_key(T(x), 8-bit expansion of entry j) over the entries j != i of subpalette p — the
 *     integer key of lib.rs:1080-1088 without the square root.  On a backdrop context the expanded subpalette counts: B is one of
 *     the other entries.  With S == 1, m(x) = 0xFFFFFFFF.
 *   COST of colour c, for every BGR555 colour, indexed u = r | g << 5 | b << 10 (as_u16, lib.rs:679-681):
 *     cost(u) = sum over the population of min(m(x), red_mean_key(T(x), 8-bit expansion of c)), in a uint64_t (below 2^45):
 *     what the pixels of subpalette p would cost if entry i were c — the k-means objective in the redmean metric.
 *   TIED SLOT of a backdrop context (palette == C, index == 0): the population is every opaque pixel, m(x) runs over the S
 *     regular entries of the pixel's own subpalette.
 *   The proxy is this key on every context, SNES_PERCEPTUAL and SNES_DITHER included: it only shortlists, the error decides.
 *   SHORTLIST of K (1..64, 0 = 16; the default mirrors --merge-shortlist and is a choice, not a measurement): the K colours
 *     lowest in (cost, u), compared lexicographically, the slot's current colour left out; candidates 0 .. K-1 in that order.  An
 *     empty population needs no rule: every cost is 0, the first K colours are scored, all tie with the incumbent.
 *   GUIDED CALL: the shortlist scored as snesimage_score_candidates scores it, acceptance as lib.rs:216-219 (best := incumbent,
 *     strict <, ascending k).  Afterwards the context is exactly what snesimage_step(SNES_METHOD_RANDOM, ...) leaves after a call
 *     that drew these K candidates: the same commit (its --dither branch, the tied spread of a backdrop slot), the same
 *     snesimage_last_step record.
 *   GUIDED SWEEP: one guided call on every slot in the order of snesimage_schedule_next (snesimage_schedule_next_backdrop on a
 *     backdrop context: the tied slot last), enqueued without a host synchronisation between them — the generator reads the
 *     palette and tile_palettes on the device, so call j + 1 sees call j's commit; the records are read back once at the end.
 *     stats: calls = windows = the slots, accepted = the calls that changed the palette, scored = useful = calls * K.
 * snesimage_guided_costs: cost(u) for all 32,768 u; synchronous; the state is unchanged.  snesimage_guided_candidates: the
 * shortlist (k * 3 raw 5-bit values) and optionally its costs; the state is unchanged.
 * The workspace (the pixel list, 512 KB at 256 x 256, and the cost table, 256 KB) is allocated by the first of these calls and
 * freed with the context; a failed allocation (SNES_ERR_HIP) leaves the context as it was.
 * Refusals: SNES_ERR_ARG for a null context or pointer, a slot out of range or k > 64; SNES_ERR_UNSUPPORTED on a SNES_NES
 * context (its NES call already scores all 56 colours of the table); SNES_ERR_STATE between the phases of a split-phase step or
 * window and on a context lent to a batch, a set or a group. */
int32_t snesimage_guided_costs(snesimage_ctx *ctx, uint32_t palette, uint32_t index, uint64_t *costs /* 32768, indexed by u */);
int32_t snesimage_guided_candidates(snesimage_ctx *ctx, uint32_t palette, uint32_t index, uint32_t k, uint8_t *rgb5 /* k*3 */, uint64_t *costs /* k, optional */);
int32_t snesimage_guided_step(snesimage_ctx *ctx, uint32_t palette, uint32_t index, uint32_t k, double *best_error, uint8_t *best_rgb5);
int32_t snesimage_guided_step_async(snesimage_ctx *ctx, uint32_t palette, uint32_t index, uint32_t k); /* results via snesimage_last_step */
int32_t snesimage_guided_sweep(snesimage_ctx *ctx, uint32_t k, snesimage_call_result *log /* optional, one per slot */, snesimage_run_stats *stats /* optional */);
/* GUIDED CALLS THROUGH THE SLOT WINDOWS (DESIGN 5f''').  n_calls guided calls of shortlist k (1..64, 0 = 16) from slot
 * (*palette, *index) on, in the order of snesimage_guided_sweep: index is the inner loop, palette the outer; on a backdrop
 * context the tied slot (sub_count, 0) comes last; behind the last slot comes (0, 0) again.  On return *palette, *index name the
 * slot of the call that would come next.  Equivalent, bit for bit, to snesimage_guided_step_async per call: the palette, the map,
 * the incumbent, the snesimage_last_step record and every log[j] with its error's bits.
 *   A guided call's shortlist depends on the palette, tile_palettes and the target image only, none of which a rejected call
 *   changes, so the calls speculate as the scheduled calls of snesimage_run_slots do: a window is the next calls in slot order,
 *   scored against the palette as it stands in one set of launches, committed in order (best := incumbent, strict <, ascending
 *   k); what lies behind the first acceptance is void and runs again in the next window.  The shortlists of a window come from
 *   one batched run of the generator (one pixel list, count and 32,768-entry table per call; integer sums throughout).
 *   window: 0 = adaptive, 1 = call by call, otherwise that many calls per launch set, at most SNES_WINDOW_MAX (default 64).  The
 *   adaptive size of guided windows is kept apart from that of snesimage_run_slots: a guided run between two scheduled runs
 *   changes neither the launch sets nor the stats of those.
 *   stats (optional) as snesimage_run_slots fills it: scored = calls taken x k, useful = calls that took effect x k, windows
 *   = launch sets (a call stepped on its own counts as one), voided = windows enqueued ahead that an acceptance voided.
 *   log (optional): n_calls records.
 *   A window ends in front of the tied slot of a backdrop context, which is stepped on its own.  Stepped call by call inside the
 *   function as well: a context the windows do not cover (snesimage_run_slots), a first call from a palette_map that is not
 *   optimize() of the palette, window = 1, and a context whose proxy is SNES_GUIDE_CIELAB (no batched CIELAB generator).
 *   The workspace of the batched generator (lists and tables for SNES_WINDOW_MAX calls: 32 MB + 16 MB at 256 x 256) is allocated
 *   by the first guided window and freed with the context, all or nothing.
 *   Refusals: those of the guided calls above and of snesimage_run_slots — SNES_ERR_ARG for a null context or pointer, a slot out
 *   of range or k > 64; SNES_ERR_UNSUPPORTED on a SNES_NES context; SNES_ERR_STATE between the phases of a split-phase step or
 *   window and on a context lent to a batch, a set or a group; SNES_ERR_HIP for a failed workspace allocation, which leaves the
 *   context as it was and usable. */
int32_t snesimage_guided_run_slots(snesimage_ctx *ctx, uint32_t n_calls, uint32_t k, uint32_t *palette, uint32_t *index, uint32_t window,
                                   snesimage_call_result *log, snesimage_run_stats *stats);
/* NOT a reference method: GUIDED CALLS OF A SET (DESIGN 5f').  The proxy above carries over to a shared-palette set without a new
 * definition: the palette and the slot are shared and the floor of a pixel depends on that pixel's own tile only.  Integers only,
 * except the objective.  For a set of F members with geometry (C, S), the shared palette and slot (p, i):
 *   POPULATION: the opaque pixels (alpha > 0) of every tile of every member whose tile_palettes value is p.  Colours are read from
 *     each member's own TARGET image T_f, so a member's ordered-dither table or level bank is followed without another argument.
 *   FLOOR m(x) and the key: exactly as above, with the shared palette; on a backdrop set the expanded subpalette counts.
 *   COST: cost(u) = sum over the members f, sum over the pixels x of member f, of min(m(x), red_mean_key(T_f(x), rgb8(u))), in a
 *     uint64_t: the sum over the members of the table above for that member.
 *   TIED SLOT of a backdrop set (palette == C, index == 0): every opaque pixel of every member; the floor runs over the S regular
 *     entries of the pixel's own subpalette.
 *   SHORTLIST: the rule above: K in 1..64 (0 = 16), lowest (cost, u), the slot's current colour left out, candidates 0 .. K-1 in
 *     that order.
 *   CAP: a set of more than 8,192 tiles in all (the character budget's cap) is refused with SNES_ERR_UNSUPPORTED.  The selection
 *     packs cost << 15 | u, so a cost must stay below 2^49; 8,192 tiles x 64 pixels x 299,505,150 (the largest key) < 2^47.2.
 *   GUIDED SET CALL: the shortlist is written into every member's candidate list; from there the call is
 *     snesimage_shared_step_async(SNES_METHOD_RANDOM, ...) word for word — scored by every member, committed once on the joint error
 *     (best := E, strict <, ascending k), the tied slot through the members' dense tied paths.  Afterwards the set is exactly what
 *     snesimage_shared_step(SNES_METHOD_RANDOM, ...) leaves after a call that drew these K candidates: every member's palette, map,
 *     incumbent and cache flags, and the record of snesimage_shared_last_step.
 *   GUIDED SET SWEEP: one guided call on every slot in the schedule's slot order, on a backdrop set the tied slot last, enqueued
 *     without a host synchronisation between them (beyond what the batched calls' ring of four argument blocks asks for); the records
 *     are read back once at the end.  stats as for snesimage_guided_sweep.
 * The workspace (the pixel list, 8 bytes x 64 per tile of the set: 4 MB at 8,192 tiles; the cost table; 256 call records) lives on
 * the set, is made by the first of these calls and freed with the set; a failed allocation (SNES_ERR_HIP) leaves the set as it was.
 * Refusals: SNES_ERR_ARG for a null set or pointer, a slot out of range (the backdrop slot of a plain set included) or k > 64;
 * SNES_ERR_UNSUPPORTED for SNES_NES members and beyond the cap; whatever every set call answers for a member changed outside the
 * set or destroyed.  A refusal leaves the set usable.  snesimage_guided_* on a lent member keeps answering SNES_ERR_STATE. */
int32_t snesimage_shared_guided_costs(snesimage_shared *set, uint32_t palette, uint32_t index, uint64_t *costs /* 32768 */);
int32_t snesimage_shared_guided_candidates(snesimage_shared *set, uint32_t palette, uint32_t index, uint32_t k, uint8_t *rgb5 /* k*3 */, uint64_t *costs /* k, optional */);
int32_t snesimage_shared_guided_step_async(snesimage_shared *set, uint32_t palette, uint32_t index, uint32_t k); /* result: snesimage_shared_last_step */
int32_t snesimage_shared_guided_step(snesimage_shared *set, uint32_t palette, uint32_t index, uint32_t k, double *error, uint8_t *best_rgb5);
int32_t snesimage_shared_guided_sweep(snesimage_shared *set, uint32_t k, snesimage_call_result *log /* optional, one per slot */, snesimage_run_stats *stats /* optional */);
/* NOT a reference method: THE CIELAB PROXY OF GUIDED CALLS (DESIGN 5f'').  On a SNES_PERCEPTUAL context the pixels choose their
 * entry by CIEDE2000, so the redmean table ranks colours by a population cost the remap does not reproduce.  This second proxy is
 * the same k-means objective in the remap's own metric, made an exact integer by fixed point.  The slot, the population, the
 * target image T, the tied slot, the set population and the shortlist rule are those above; only the distance changes:
 *   DISTANCE d(c, x) = ciede2000(Lab(rgb8(c)), Lab(T(x))) in f32: entry first, target second, through the sRGB table and the Lab
 *     pipeline of the remap (lib.rs:1090-1100: distance_cielab(entry, target)).
 *   FIXED POINT q(d) = min((uint32_t)(d * 65536.0f), 0xFFFFFF).  The product by 2^16 is exact in f32, so the truncation is exact; q
 *     is monotone, so q(min) = min(q).
 *   FLOOR m(x) = the minimum of q(d(entry j, x)) over the entries j != i of the subpalette (the expanded one on a backdrop
 *     context); 0xFFFFFFFF with S == 1.  A transparent pixel adds 0 to every sum.
 *   COST cost(u) = sum over the population of min(m(x), q(d(c_u, x))) in a uint64_t, in Q16 units of dE00: at most
 *     2^24 * 2^19 = 2^43 for a set of 8,192 tiles.  A set's table is the integer sum over all its members' tiles.
 * snesimage_set_guided_proxy selects the table that snesimage_guided_costs / _candidates / _step(_async) / _sweep use:
 * SNES_GUIDE_REDMEAN (the default) or SNES_GUIDE_CIELAB.  Legal on every context but SNES_NES (SNES_ERR_UNSUPPORTED), perceptual or
 * not; SNES_ERR_ARG for another value; SNES_ERR_STATE between the phases of a split-phase step or window and on a context lent to a
 * batch, a set or a group, as snesimage_set_ordered_dither refuses.  A refusal leaves the setting as it was.  The state of the
 * context is not touched; the CIELAB pixel list (16 bytes a pixel: 1 MB at 256 x 256) is allocated by the first guided call under
 * SNES_GUIDE_CIELAB.  A context that never selects SNES_GUIDE_CIELAB issues exactly the launches it issued before.
 * snesimage_shared_set_guided_proxy does the same for snesimage_shared_guided_*: the set's setting is its own, the members' settings
 * are neither read nor written (list: 8 MB at 8,192 tiles).  It refuses what every set call refuses, SNES_NES members and a bad value. */
enum { SNES_GUIDE_REDMEAN = 0, SNES_GUIDE_CIELAB = 1 };
int32_t snesimage_set_guided_proxy(snesimage_ctx *ctx, uint32_t proxy);
int32_t snesimage_get_guided_proxy(snesimage_ctx *ctx, uint32_t *proxy);
int32_t snesimage_shared_set_guided_proxy(snesimage_shared *set, uint32_t proxy);
int32_t snesimage_shared_get_guided_proxy(snesimage_shared *set, uint32_t *proxy);
/* GUIDED CALLS OF A SET THROUGH THE SLOT WINDOWS (DESIGN 5f'''').  n_calls guided set calls of shortlist k (1..64, 0 = 16) from
 * slot (*palette, *index) on, in the order of snesimage_shared_guided_sweep: index is the inner loop, palette the outer; on a
 * backdrop set the tied slot (sub_count, 0) comes last; behind the last slot comes (0, 0) again.  On return *palette, *index name
 * the slot behind the last call that took effect.  Equivalent, bit for bit and for every `window`, to
 * snesimage_shared_guided_step_async per call: every member's palette, map and incumbent, the set's record
 * (snesimage_shared_last_step) and every log[j] with its error's bits.
 *   A rejected guided set call changes nothing that a shortlist or a score reads, so a guided window is a window of
 *   snesimage_shared_run_slots whose candidate lists are shortlists: the next calls in slot order, scored by every member against
 *   the palette as it stands in one set of launches, committed once on the joint error in order (best := E, strict <, ascending
 *   k); what lies behind the first acceptance runs again in the next window.  One window is in flight at a time: voided stays 0.
 *   THE WINDOW'S GENERATOR does not repeat a subpalette's work for each of its entries.  For a pixel x of subpalette p, over the
 *   entries of the (expanded) subpalette: a(x) = the lowest key, j*(x) = the first entry that reaches it, b(x) = the lowest key
 *   over j != j*(x) (0xFFFFFFFF with one entry).  The floor of slot (p, i) is b(x) where j*(x) == i, else a(x), so
 *     A_p(u) = sum over p's population of min(a, key(x, u)),
 *     D_{p,i}(u) = sum over the pixels with j* == i of min(b, key(x, u)) - min(a, key(x, u)),    cost_{p,i}(u) = A_p(u) + D_{p,i}(u)
 *   in integers and exactly: A once per subpalette and window, D once per call over the pixels whose nearest entry is the call's.
 *   The tables and the shortlists equal those of snesimage_shared_guided_costs / _candidates bit for bit.
 *   window: 0 = adaptive, 1 = call by call, otherwise that many calls per launch set, at most SNES_WINDOW_MAX / F.  The adaptive
 *   size is kept apart from that of snesimage_shared_run_slots: a guided run between two scheduled runs changes neither the launch
 *   sets nor the stats of those.  stats and log (both optional) as snesimage_guided_run_slots fills them.
 *   Stepped call by call inside the function: the tied slot (a window ends in front of it), window = 1, a set of more than
 *   SNES_WINDOW_MAX / 2 members, members whose maps are not optimize() of the palette, and a set whose proxy is SNES_GUIDE_CIELAB.
 *   The generator's workspace (per call of SNES_WINDOW_MAX / F: 16 bytes x 64 per tile of the set and a table; per subpalette of a
 *   window: 8 bytes x 64 per tile and a table) is allocated by the first guided window and freed with the set, all or nothing.
 *   Refusals: those of snesimage_shared_guided_step and of snesimage_shared_run_slots; SNES_ERR_HIP for a failed workspace
 *   allocation.  A refusal leaves the set as it was and usable. */
int32_t snesimage_shared_guided_run_slots(snesimage_shared *set, uint32_t n_calls, uint32_t k, uint32_t *palette, uint32_t *index, uint32_t window,
                                          snesimage_call_result *log, snesimage_run_stats *stats);
int32_t snesimage_get_palette_map(snesimage_ctx *ctx, uint8_t *out /*w*h*/);
int32_t snesimage_set_palette_map(snesimage_ctx *ctx, const uint8_t *in);
int32_t snesimage_as_rgba(snesimage_ctx *ctx, uint8_t *out /*w*h*4; lib.rs:550-577*/);
/* as_json().to_string() — lib.rs:579-625, 1002.  Returns the byte count needed including the
 * terminating NUL (negative on error) and writes at most cap bytes. */
int64_t snesimage_as_json(snesimage_ctx *ctx, char *out, int64_t cap);

/* Candidate generator used by SNES_METHOD_RANDOM (host helper; replaces the reference's unseeded
 * rand::rng() of lib.rs:201-208). */
void snesimage_random_candidates(uint64_t seed, uint64_t step_id, uint32_t n, uint8_t *rgb5);
/* Slot scheduler of lib.rs:881-933 (host helper): reports the method for the current slot and
 * advances (palette, index, channel, step). */
void snesimage_schedule_next(uint32_t sub_count, uint32_t sub_size, int32_t nes, uint32_t *palette,
                             uint32_t *index, uint32_t *channel, uint32_t *step, uint32_t *method);

/* The scheduler of a backdrop context: the reference's with one more slot per sweep — behind (sub_count - 1, sub_size - 1)
 * comes the backdrop slot (sub_count, 0), then the wrap to the next step; the backdrop slot gets three channel calls in a
 * channel sweep like every entry.  Equivalently snesimage_schedule_next for geometry (1, sub_count*sub_size + 1) with linear
 * index L: L < sub_count*sub_size is (L / sub_size, L % sub_size), L == sub_count*sub_size the backdrop slot. */
void snesimage_schedule_next_backdrop(uint32_t sub_count, uint32_t sub_size, int32_t nes, uint32_t *palette,
                                      uint32_t *index, uint32_t *channel, uint32_t *step, uint32_t *method);

/* Device-side evaluation of the deterministic math used by the kernels, for bit-parity tests:
 * op 0 sin, 1 cos, 2 exp(x<=0), 3 cbrt, 4 atan2(y,x), 5 CIEDE2000(lab x[3i..], lab y[3i..]),
 * 6 sRGB8->Lab (x holds r,g,b as floats, out 3 per item),
 * 7 and 8 the two sure "no"s of the CIEDE2000 win test for candidate lab x[3i..] and target lab y[3i..], with the bound
 * set to the pair's own distance d = CIEDE2000(x, y) computed on the device: 7 the lightness test, 8 the lightness and
 * a-b plane test (1.0f = "cannot beat d", 0.0f otherwise; a correct test never says 1.0f at a pair's own distance).
 * Any other op is SNES_ERR_ARG.  Host pointers. */
int32_t snesimage_debug_math(int32_t device, int32_t op, const float *x, const float *y, uint32_t n,
                             float *out);
/* Fault injection for tests: the (n+1)-th workspace allocation made by the library from now on fails as if the
 * device were out of memory (n < 0 switches the hook off).  A failed grow returns SNES_ERR_HIP and leaves the context
 * usable: the next call allocates afresh. */
void snesimage_debug_fail_alloc(int32_t n);
/* Test hook: while on (non-zero), the group-sparse path's per-candidate storage is filled with 0xff bytes (a NaN in every
 * float) when it is allocated, so that a read of anything no kernel wrote shows in the results instead of reading the
 * zeros a fresh allocation often holds.  Applies to storage allocated after the call. */
void snesimage_debug_poison_alloc(int32_t on);
/* Test hook: the shortlists snesimage_guided_run_slots scored.  While the capture is on (non-zero), every run keeps, for each
 * call that took effect, the k candidates the call scored, read back from where the scorer read them — the window's candidate
 * list for a call of a window (the calls voided behind an acceptance are not kept: they run again), the context's for a
 * call stepped on its own; a run replaces what the run before it kept, and the read-back synchronises, so the capture is for
 * tests.  snesimage_debug_guided_shortlists copies them out: *n_calls and *k of the last captured run, and, if rgb5 is not
 * null and holds cap >= n_calls * k * 3 bytes, the raw 5-bit triples, call after call, candidate 0 first (SNES_ERR_ARG for
 * a null context or a buffer that is too short). */
int32_t snesimage_debug_guided_capture(snesimage_ctx *ctx, int32_t on);
int32_t snesimage_debug_guided_shortlists(snesimage_ctx *ctx, uint8_t *rgb5, uint32_t cap, uint32_t *n_calls, uint32_t *k);
/* The same two hooks for snesimage_shared_guided_run_slots: the lists the members' scorers read, for every call that took effect. */
int32_t snesimage_shared_debug_guided_capture(snesimage_shared *set, int32_t on);
int32_t snesimage_shared_debug_guided_shortlists(snesimage_shared *set, uint8_t *rgb5, uint32_t cap, uint32_t *n_calls, uint32_t *k);
/* Test hook: the tables of the guided windows' generator.  Runs the generator of one window whose calls are the n given slots
 * (1 <= n <= SNES_WINDOW_MAX / F; regular slots; a slot may repeat) without scoring or committing anything and returns each
 * call's final table, costs[j * 32768 + u] = A + D of call j.  The state is left unchanged.  SNES_ERR_ARG for a null pointer, a
 * slot out of range, the tied slot or a bad n; SNES_ERR_UNSUPPORTED under SNES_GUIDE_CIELAB and where the guided set calls are. */
int32_t snesimage_shared_debug_guided_window_costs(snesimage_shared *set, const uint32_t *palettes, const uint32_t *indices, uint32_t n, uint64_t *costs /* n*32768 */);
/* Launch timing by the library's own HIP events on the stream each launch group runs on (bench.py's roofline leg).
 * While enabled, every scoring launch group records events; timing_read() returns summed milliseconds:
 *   ms3[0] = the whole launch group (all kernels that score one chunk of candidates);
 *   ms3[1] = the H pass: k_sparse_h2 + k_sparse_h (wide and narrow scales) on the group-sparse path, k_hpass* at scale 0 otherwise;
 *   ms3[2] = the V pass, the dominant kernel: k_sparse_v2 alone (one launch, the scales at least 64 wide; the wait for
 *            B's checkpoints and k_sparse_order come before the opening event) on the group-sparse path — for launch groups
 *            of 1,024 candidates and more, which run on two streams, the launch of scale 0 (three quarters of the V pass)
 *            on its stream, with the other stream's kernels resident beside it — k_vpass* at scale 0 otherwise;
 * plus the number of launch groups and the candidates they scored since timing was enabled.
 * on = 1: all three brackets — six event records per launch group, each a ~4 us bubble in the stream (25 us per group: 1.5 % of a
 * 4,096-candidate group, 9 % of a 64-candidate one; profiles/r4_timing_cost.py).  on = 2: the V pass's bracket only (ms3[0] and
 * ms3[1] stay 0): what bench.py keeps on over its timed region.  on = 0: off. */
int32_t snesimage_timing_enable(snesimage_ctx *ctx, int32_t on);
int32_t snesimage_timing_read(snesimage_ctx *ctx, double *ms3, uint64_t *launches,
                              uint64_t *candidates);

const char *snesimage_last_error(void);
const char *snesimage_version(void);

#ifdef __cplusplus
}
#endif
#endif
