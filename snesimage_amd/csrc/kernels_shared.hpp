// snesimage_amd/csrc/kernels_shared.hpp — one palette shared by several images (a set, shared_host.inc).
// A set call is an image batch's call (kernels_batch.hpp) with one candidate list for every member; only the commit
// differs: it decides once, on the joint error E_k = sum over the members of their errors e_{i,k}, and writes that
// decision into every member.  Sums run in member order, left to right, with plain `+` (the build has
// -ffp-contract=off), so a set of one member commits exactly what kb_commit / k_commit would.
#pragma once
#include "kernels_batch.hpp"

namespace snes {

// Joint commit of a set of K members (their arguments in A, every member's call of A[0].n candidates already scored into
// its own a.errors).  The lexicographic (E, k) minimum of commit_body is accepted iff it is strictly below the joint
// incumbent sum_i *inc_err_i (the random and channel methods, lib.rs:216-219) or always (the NES method, lib.rs:250); a NaN
// in any member's e_{i,k} makes E_k NaN, which never wins.  Every member then takes the decision through commit_apply:
// the slot's colour and palette-table rows, its own e_{i,k*} as its incumbent, its own record (the member's error).
// *joint: the set's record, error = E after the call (the members' new incumbents summed in member order).
__global__ __launch_bounds__(256) void ks_commit(const BatchArgs *__restrict__ A, int K, StepResult *__restrict__ joint) {
    __shared__ double s_e[256];
    __shared__ int s_k[256];
    const int t = threadIdx.x, n = A[0].n;
    double be = __longlong_as_double(0x7ff0000000000000ll); int bk = 0x7fffffff;
    for (int k = t; k < n; k += 256) {
        double e = A[0].errors[k];
        for (int i = 1; i < K; i++) e = e + A[i].errors[k];
        if (e < be) { be = e; bk = k; }
    }
    s_e[t] = be; s_k[t] = bk;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (t < st) {
            const double e2 = s_e[t + st]; const int k2 = s_k[t + st];
            if (e2 < s_e[t] || (e2 == s_e[t] && k2 < s_k[t])) { s_e[t] = e2; s_k[t] = k2; }
        }
        __syncthreads();
    }
    if (t != 0) return;
    // the decision (commit_decide's rule on the sums); a handful of dependent loads and stores per member below
    const int nes = A[0].nes;
    double inc = *A[0].inc_err;
    for (int i = 1; i < K; i++) inc = inc + *A[i].inc_err;
    const double start = nes ? 1.7976931348623157e308 : inc;
    int best_k = -1;
    if (s_k[0] != 0x7fffffff && s_e[0] < start) best_k = s_k[0];
    const bool took = best_k >= 0;
    if (nes && best_k < 0) best_k = 0; // best_index = 0 (lib.rs:249): the colour is taken, no incumbent moves
    double E = 0.0;
    for (int i = 0; i < K; i++) {
        const BatchArgs &a = A[i];
        commit_apply(took ? a.errors[best_k] : 1.7976931348623157e308, best_k, a.cand, a.colors, a.slot, a.inc_err, a.last, a.T);
        E = i == 0 ? a.last->error : E + a.last->error;
    }
    StepResult r = *A[0].last;
    r.error = E;
    *joint = r;
}

// ---- slot windows of a set (snesimage_shared_run_slots, shared_window_host.inc) --------------------------------------
// A window of K calls over F members is one set of the batched launches with F * G "images": G groups of calls (one call,
// or the up to three channel calls of one entry behind one base image), every group once per member.  The argument blocks
// are member-major, A[i * G + g]; member i's errors of call j sit at errors[(i * K + j) * stride + k].  Every member of a
// call scores the call's one candidate list, cand + 3 * j * stride.
//
// ksw_commit is kw_commit's in-order walk with ks_commit's rule: per call j and candidate k the joint error
// E[j][k] = e[0][j][k] + e[1][j][k] + ... (member order, left to right, plain `+`: the order ks_commit and the host use),
// per call its lexicographic (E, k) minimum — sixteen lanes per call, a shuffle reduction, the minima staged in LDS — and
// the joint incumbent inc_0 + inc_1 + ... in the same order.  Random and channel calls are all measured against that one
// incumbent until the first of them accepts, so which call accepts first is a parallel minimum over the calls; the calls
// before it log "nothing accepted", the calls behind it are void.  NES calls always take their argmin and are applied in
// sequence up to the first one that changed the colour.  The accepting call is applied to every member through
// commit_apply (member i's incumbent := its own e[i][j*][k*]); a window that accepted nothing leaves in every member's
// record what ks_commit leaves after its last call.  log[j] / *joint: the set's record after call j (error = E).
__global__ __launch_bounds__(1024) void ksw_commit(const WindowSlot *__restrict__ S, int K, int stride, int F, int G, const BatchArgs *__restrict__ A, const double *__restrict__ errors,
                                                  const uint8_t *__restrict__ cand, StepResult *__restrict__ joint, WindowResult *__restrict__ res, StepResult *__restrict__ log) {
    __shared__ double s_e[kMaxWindow];
    __shared__ int s_k[kMaxWindow];
    __shared__ int s_first;
    const double kInf = __longlong_as_double(0x7ff0000000000000ll), kMax = 1.7976931348623157e308;
    const int l16 = threadIdx.x & 15, q = threadIdx.x >> 4; // sixteen lanes per call, 64 calls at a time
    const size_t member_stride = (size_t)K * stride;
    for (int j = q; j < K; j += 64) {
        const int n = S[j].n;
        const double *e0 = errors + (size_t)j * stride;
        double be = kInf; int bk = 0x7fffffff;
        for (int k = l16; k < n; k += 16) {
            double e = e0[k];
            for (int i = 1; i < F; i++) e = e + e0[(size_t)i * member_stride + k];
            if (e < be) { be = e; bk = k; } // NaN never wins, as in the reference
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {
            const double e2 = __shfl_xor(be, o); const int k2 = __shfl_xor(bk, o);
            if (e2 < be || (e2 == be && k2 < bk)) { be = e2; bk = k2; }
        }
        if (l16 == 0) { s_e[j] = be; s_k[j] = bk; }
    }
    if (threadIdx.x == 0) s_first = K;
    __syncthreads();
    const uint8_t *colors0 = A[0].colors; // the members hold the same palette: the records read member 0's
    int consumed = 0, accepted = 0;
    if (K > 0 && !S[0].nes) {
        double inc = *A[0].inc_err;
        for (int i = 1; i < F; i++) inc = inc + *A[(size_t)i * G].inc_err;
        for (int j = threadIdx.x; j < K; j += 1024) if (s_k[j] != 0x7fffffff && s_e[j] < inc) atomicMin(&s_first, j);
        __syncthreads();
        const int first = s_first;
        for (int j = threadIdx.x; j < first; j += 1024) {
            const int slot = S[j].slot;
            StepResult r; r.error = inc; r.best_k = -1; r.rgb5[0] = colors0[3 * slot]; r.rgb5[1] = colors0[3 * slot + 1]; r.rgb5[2] = colors0[3 * slot + 2]; r.changed = 0;
            log[j] = r;
        }
        __syncthreads(); // the records above read the palette; the accepting call below rewrites its slot
        if (threadIdx.x != 0) return;
        const int j = first < K ? first : K - 1, best_k = first < K ? s_k[first] : -1; // the window's last call that took effect, and its winner (none: what ks_commit records)
        const uint8_t *cj = cand + 3 * (size_t)j * stride;
        double E = 0.0;
        for (int i = 0; i < F; i++) {
            const BatchArgs &a = A[(size_t)i * G];
            commit_apply(best_k >= 0 ? errors[(size_t)i * member_stride + (size_t)j * stride + best_k] : kMax, best_k, cj, a.colors, S[j].slot, a.inc_err, a.last, a.T);
            E = i == 0 ? a.last->error : E + a.last->error;
        }
        StepResult r = *A[0].last;
        r.error = E;
        log[j] = r; *joint = r;
        consumed = j + 1; accepted = first < K ? 1 : 0;
    } else {
        if (threadIdx.x != 0) return;
        for (int j = 0; j < K && !accepted; j++) { // ks_commit's NES branch, call after call
            int best_k = -1;
            if (s_k[j] != 0x7fffffff && s_e[j] < kMax) best_k = s_k[j];
            const bool took = best_k >= 0;
            if (best_k < 0) best_k = 0; // best_index = 0 (lib.rs:249)
            const uint8_t *cj = cand + 3 * (size_t)j * stride;
            double E = 0.0;
            for (int i = 0; i < F; i++) {
                const BatchArgs &a = A[(size_t)i * G];
                commit_apply(took ? errors[(size_t)i * member_stride + (size_t)j * stride + best_k] : kMax, best_k, cj, a.colors, S[j].slot, a.inc_err, a.last, a.T);
                E = i == 0 ? a.last->error : E + a.last->error;
            }
            StepResult r = *A[0].last;
            r.error = E;
            log[j] = r; *joint = r;
            consumed = j + 1;
            accepted = r.changed ? 1 : 0;
        }
    }
    res->consumed = consumed; res->accepted = accepted;
}

// --dither: every member's palette_map of the committed state is the winner's resumed run in that member's own slot
// context (kw_take_map for one image).  grid.x = member; nothing accepted: the stored maps stand.
__global__ __launch_bounds__(1024) void ksw_take_map(const BatchArgs *__restrict__ A, int G, const WindowSlot *__restrict__ S, const WindowResult *__restrict__ res, const StepResult *__restrict__ log, int npx) {
    if (!res->accepted) return;
    const int j = res->consumed - 1, k = log[j].best_k;
    if (k < 0) return;
    const BatchArgs &a = A[(size_t)blockIdx.x * G + S[j].member];
    const uint4 *src = reinterpret_cast<const uint4 *>(a.Pc.maps + (size_t)(S[j].cand0 + k) * npx);
    uint4 *dst = reinterpret_cast<uint4 *>(a.map);
    for (int i = threadIdx.x; i < npx / 16; i += 1024) dst[i] = src[i];
}

// ---- the backdrop colour of a set (snesimage_shared_create_backdrop, shared_host.inc; DESIGN §5c'') -------------------
// A call on the backdrop slot of a set: every member scored the one candidate list on its own stream through its dense tied
// path (pack mode 3) into its own error vector; this is the one commit behind them.  The joint (E, k) minimum and the decision
// are ks_commit's, word for word; every member then takes the decision as k_commit leaves a tied call of a single context:
// commit_apply on the first tied entry `slot` with the member's own e_{i,k*} as its incumbent, then tied_spread over the
// member's tied_count tied entries, tied_stride apart (the colour and its rows of pal_rgb8 / pal_lin / pal_xyb / pal_lab).
struct TiedMember { const double *errors; const uint8_t *cand; uint8_t *colors; double *inc_err; StepResult *last; PaletteTables T; };
__global__ __launch_bounds__(256) void ks_commit_tied(const TiedMember *__restrict__ A, int K, int n, int nes, int slot, int tied_count, int tied_stride, StepResult *__restrict__ joint) {
    __shared__ double s_e[256];
    __shared__ int s_k[256];
    const int t = threadIdx.x;
    double be = __longlong_as_double(0x7ff0000000000000ll); int bk = 0x7fffffff;
    for (int k = t; k < n; k += 256) {
        double e = A[0].errors[k];
        for (int i = 1; i < K; i++) e = e + A[i].errors[k];
        if (e < be) { be = e; bk = k; } // NaN never wins, as in the reference
    }
    s_e[t] = be; s_k[t] = bk;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (t < st) {
            const double e2 = s_e[t + st]; const int k2 = s_k[t + st];
            if (e2 < s_e[t] || (e2 == s_e[t] && k2 < s_k[t])) { s_e[t] = e2; s_k[t] = k2; }
        }
        __syncthreads();
    }
    if (t != 0) return;
    double inc = *A[0].inc_err;
    for (int i = 1; i < K; i++) inc = inc + *A[i].inc_err;
    const double start = nes ? 1.7976931348623157e308 : inc;
    int best_k = -1;
    if (s_k[0] != 0x7fffffff && s_e[0] < start) best_k = s_k[0];
    const bool took = best_k >= 0;
    if (nes && best_k < 0) best_k = 0; // best_index = 0 (lib.rs:249)
    double E = 0.0;
    for (int i = 0; i < K; i++) {
        const TiedMember &a = A[i];
        commit_apply(took ? a.errors[best_k] : 1.7976931348623157e308, best_k, a.cand, a.colors, slot, a.inc_err, a.last, a.T);
        if (best_k >= 0 && tied_count > 1) tied_spread(a.colors, slot, tied_count, tied_stride, a.T);
        E = i == 0 ? a.last->error : E + a.last->error;
    }
    StepResult r = *A[0].last;
    r.error = E;
    *joint = r;
}

// Joint sum for explicit candidate lists: out[k] = errs[0][k] + errs[1][k] + ... in member order.
__global__ __launch_bounds__(256) void ks_sum(const double *const *__restrict__ errs, int K, int n, double *__restrict__ out) {
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= n) return;
    double e = errs[0][k];
    for (int i = 1; i < K; i++) e = e + errs[i][k];
    out[k] = e;
}

} // namespace snes
