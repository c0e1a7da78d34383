// smpl_amd/csrc/path_kernels.h -- path post-processing for a batch of paths (smplx_post_process_paths; host: path_multi.h).
// Owns: k_shortcut (shortcut_run of path_tools.h -- shortcut.hpp:110-286 with the joint-space generator
// post_processing.cpp:100-127, look-ahead 1 -- one workgroup per path, run to the end on the device), k_paths_valid
// (isStateValid of the rows of many paths in one launch, each path against its own space: the two InterpolatePath
// passes) and k_path_waypoints (test hook: the joint values k_shortcut's lanes stage for an edge).
// Everything is built from config_checks.h (edge_waypoint_count, config_valid) and det_math.h; nothing is restated but
// the greedy loop itself and PathTools::distance.
//
// k_shortcut, one block of BLOCK lanes per path.  The reference's loop is a chain of edge questions -- "is (a, b)
// valid?" -- each followed by a decision that names the next question.  A trip of the kernel's loop is one question:
//   all lanes   read the question (a, b) from the LDS record; W = edge_waypoint_count(a, b), the same in every lane
//   lane l      checks waypoints l, l + BLOCK, ... of the edge through config_valid over its own LDS scratch, as the
//               lanes of k_true_cost do; a lane that finds a collision raises the record's `bad` word
//   barrier
//   lane 0      the edge is valid iff no lane raised `bad` (collision_space.cpp:561-577; W == 0 asks nothing and is
//               valid).  It takes the greedy decision with the reference's arithmetic -- the edge's cost is
//               PathTools::distance, the accumulated costs are the host's (path_multi.h uploads accum[]) -- appends the
//               indices the decision emits to the path's keep list and writes the next question, or `done`
//   barrier
// so every lane takes the same trip through every barrier.  The output of a shortcut is a subsequence of its input:
// the kernel returns indices, the host gathers the points.
// Trips: a question of kind 1 (extend: (start, end + 1)) advances `end` whatever its answer; a question of kind 0
// (restart: (start, end)) follows the first question or a failed extension.  At most P - 1 of the first and P of the
// second: a block that is about to start trip 2P + 3 has met a bug, sets its path's error word and stops.
#pragma once

#include "config_checks.h"

// the LDS record of a k_shortcut block: the question of the next trip and the reference loop's variables
struct ShortcutRec {
    int a, b;            // the candidate edge (indices into the path)
    int kind;            // 0: the segment's first edge (start, end); 1: the extension (start, end + 1)
    int done;            // the loop has ended, the keep list is complete
    int bad;             // some lane found a waypoint of (a, b) in collision
    int start, end;      // shortcut.hpp's segment
    int best_last, best_direct;
    int nkeep;           // indices emitted so far
    double best_cost;
};

// PathTools::distance (post_processing.cpp:52-67): the same sum in the same order
__device__ __forceinline__ double path_distance(const ModelLds* __restrict__ M, const double* __restrict__ from,
                                                const double* __restrict__ to)
{
    double dist = 0.0;
    const int nv = MV_NVARS(M);
    MV_UNROLL
    for (int v = 0; v < nv; ++v) {
        if (MV_TYPE(M, v) == SMPLX_JT_CONTINUOUS) dist += fabs(smplx_shortest_angle_diff(to[v], from[v]));
        else dist += fabs(to[v] - from[v]);
    }
    return dist;
}

// waypoint j of W on the edge a -> b, as config_valid's stage_config takes it: alpha = j / (W - 1) in the host's
// arithmetic (smplx_cc_interpolate: (double)j * (1.0 / (double)(W - 1)))
__device__ __forceinline__ EdgeRef path_waypoint(const double* __restrict__ a, const double* __restrict__ b, int j, int W)
{
    EdgeRef e;
    e.start = a;
    e.finish = b;
    e.alpha = (double)j * (1.0 / (double)(W - 1));
    return e;
}

// the emit_best of shortcut_run: indices instead of points.  A list longer than the path cannot happen (the indices
// ascend); it is counted all the same and the caller reports it
__device__ __forceinline__ int shortcut_emit(int* __restrict__ keep, int P, int nk, int start, int best_last, int best_direct)
{
    if (best_direct) { if (nk < P) keep[nk] = best_last; return nk + 1; }
    for (int i = start + 1; i <= best_last; ++i) { if (nk < P) keep[nk] = i; ++nk; }
    return nk;
}

// pts: the points of all paths back to back, first[k] .. first[k + 1] those of path k; accum: per point, the accumulated
// cost from its path's first point (host arithmetic); keep: per point, room for path k's list at first[k]; nkeep, err,
// checked: per path.  err: 0, 1 = trip bound exceeded, 2 = keep list overflow.  checked: waypoints dealt to the lanes.
extern "C" __global__ void __launch_bounds__(BLOCK, 2)   // >= 2 waves per SIMD: at most 256 VGPRs, whichever compiler builds it
k_shortcut(const SmplxSpaceDev* const* __restrict__ stab, const double* __restrict__ pts, const int* __restrict__ first,
           const double* __restrict__ accum, int* __restrict__ keep_all, int* __restrict__ nkeep, int* __restrict__ err,
           long long* __restrict__ checked)
{
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ ShortcutRec R;
    const int k = blockIdx.x;
    const SmplxSpaceDev* __restrict__ S = stab[k];
    ModelLds Mv;
#ifdef SMPLX_CONST_MODEL
    constexpr bool RS = true;      // as k_state_valid
#else
    constexpr bool RS = false;
#endif
    ThreadLds L = setup_lds(S, smem, &Mv, BLOCK, !RS);
    const ModelLds* M = &Mv;
    const int nv = MV_NVARS(M);
    const int p0 = first[k];
    const int P = first[k + 1] - p0;
    const double* __restrict__ path = pts + (size_t)p0 * nv;
    const double* __restrict__ acc = accum + p0;
    int* __restrict__ keep = keep_all + p0;
    if (P < 2) {                   // (uniform) shortcut_path: nothing to do
        if (threadIdx.x == 0) { if (P == 1) keep[0] = 0; nkeep[k] = P; err[k] = 0; checked[k] = 0; }
        return;
    }
    if (threadIdx.x == 0) {
        R.a = 0; R.b = 1; R.kind = 0; R.done = 0; R.bad = 0;
        R.start = 0; R.end = 1; R.best_last = 1; R.best_direct = 0;
        R.best_cost = acc[1] - acc[0];
        keep[0] = 0;
        R.nkeep = 1;
    }
    __syncthreads();
    const SmplxGridDev grid = S->grid;
    const int max_trips = 2 * P + 2;
    int trips = 0, failure = 0;
    long long dealt = 0;
    for (;;) {
        const int a = R.a, b = R.b;
        if (R.done) break;
        if (++trips > max_trips) { failure = 1; break; }      // (uniform: every lane counts alike)
        const double* __restrict__ qa = path + (size_t)a * nv;
        const double* __restrict__ qb = path + (size_t)b * nv;
        const int W = edge_waypoint_count(M, qa, qb);
        dealt += W;
        int lk = 0;
        for (int j = threadIdx.x; j < W; j += BLOCK) {
            const EdgeRef e = path_waypoint(qa, qb, j, W);
            if (!config_valid<RS>(M, L, grid, e, lk)) { R.bad = 1; break; }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const bool valid = R.bad == 0;
            int start = R.start, end = R.end, best_last = R.best_last, best_direct = R.best_direct, nk = R.nkeep;
            double best_cost = R.best_cost;
            bool restart = false;
            if (R.kind == 1) {
                // shortcut.hpp's loop body with look == 1
                double new_cost = best_cost + (acc[end + 1] - acc[end]);
                bool improved = false;
                if (valid) {
                    const double cost = path_distance(M, path + (size_t)start * nv, path + (size_t)(end + 1) * nv);
                    if (cost <= new_cost) { improved = true; best_direct = 1; best_last = end + 1; new_cost = cost; }
                }
                best_cost = new_cost;
                if (improved) {
                    end += 1;
                } else {
                    nk = shortcut_emit(keep, P, nk, start, best_last, best_direct);
                    start = end;
                    end += 1;
                    best_direct = 0;
                    best_last = end;
                    best_cost = acc[end] - acc[start];
                    restart = true;
                }
            } else if (valid) {
                const double cost = path_distance(M, path + (size_t)start * nv, path + (size_t)end * nv);
                if (cost <= best_cost) { best_direct = 1; best_cost = cost; }
            }
            if (restart) {
                R.a = start; R.b = end; R.kind = 0;
            } else if (P - end - 1 <= 0) {      // look == 0: end = P, the loop ends
                nk = shortcut_emit(keep, P, nk, start, best_last, best_direct);
                R.done = 1;
            } else {
                R.a = start; R.b = end + 1; R.kind = 1;
            }
            R.start = start; R.end = end; R.best_last = best_last; R.best_direct = best_direct; R.nkeep = nk;
            R.best_cost = best_cost;
            R.bad = 0;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int nk = R.nkeep;
        nkeep[k] = nk;
        err[k] = failure ? 1 : (nk > P ? 2 : 0);
        checked[k] = dealt;
    }
}

// isStateValid of the rows of many paths in one launch.  blocks: per block (path, first row, rows <= BLOCK); the rows of a
// block belong to one path and are checked against stab[path], as states (alpha == 0): the waypoints the host
// interpolated, the doubles the single-path call uploads.
extern "C" __global__ void __launch_bounds__(BLOCK, 2)   // >= 2 waves per SIMD: at most 256 VGPRs, whichever compiler builds it
k_paths_valid(const SmplxSpaceDev* const* __restrict__ stab, const int* __restrict__ blocks, const double* __restrict__ Q,
              unsigned char* __restrict__ out)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int path = blocks[3 * blockIdx.x], row0 = blocks[3 * blockIdx.x + 1], rows = blocks[3 * blockIdx.x + 2];
    const SmplxSpaceDev* __restrict__ S = stab[path];
    ModelLds Mv;
#ifdef SMPLX_CONST_MODEL
    constexpr bool RS = true;      // as k_state_valid
#else
    constexpr bool RS = false;
#endif
    ThreadLds L = setup_lds(S, smem, &Mv, BLOCK, !RS);
    const ModelLds* M = &Mv;
    if ((int)threadIdx.x >= rows) return;
    const size_t i = (size_t)row0 + threadIdx.x;
    EdgeRef e;
    e.start = Q + i * MV_NVARS(M); e.finish = e.start; e.alpha = 0.0;
    int lk = 0;
    const SmplxGridDev grid = S->grid;
    out[i] = config_valid<RS>(M, L, grid, e, lk) ? 1 : 0;
}

// test hook (test_hooks.h smplx_test_path_waypoints): one block per edge A[i] -> B[i]; its lanes take the waypoints as
// k_shortcut's do and write what stage_config staged for each.  first: n + 1 row offsets into out, the host's counts;
// nothing is written past an edge's rows.
extern "C" __global__ void __launch_bounds__(BLOCK)
k_path_waypoints(const SmplxSpaceDev* __restrict__ S, const double* __restrict__ A, const double* __restrict__ B,
                 const int* __restrict__ first, double* __restrict__ out, int* __restrict__ out_count)
{
    extern __shared__ __align__(16) unsigned char smem[];
    ModelLds Mv;
    ThreadLds L = setup_lds(S, smem, &Mv);
    const ModelLds* M = &Mv;
    const int nv = MV_NVARS(M);
    const int i = blockIdx.x;
    const double* __restrict__ qa = A + (size_t)i * nv;
    const double* __restrict__ qb = B + (size_t)i * nv;
    const int W = edge_waypoint_count(M, qa, qb);
    if (threadIdx.x == 0) out_count[i] = W;
    const int rows = first[i + 1] - first[i];
    for (int j = threadIdx.x; j < W && j < rows; j += BLOCK) {
        const EdgeRef e = path_waypoint(qa, qb, j, W);
        stage_config(M, L, e);
        for (int v = 0; v < nv; ++v) out[((size_t)first[i] + j) * nv + v] = lds_d(L, L.q_base + v);
    }
}
