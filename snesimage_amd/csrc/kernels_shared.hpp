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

// Joint sum for explicit candidate lists: out[k] = errs[0][k] + errs[1][k] + ... in member order.
__global__ __launch_bounds__(256) void ks_sum(const double *const *__restrict__ errs, int K, int n, double *__restrict__ out) {
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= n) return;
    double e = errs[0][k];
    for (int i = 1; i < K; i++) e = e + errs[i][k];
    out[k] = e;
}

} // namespace snes
