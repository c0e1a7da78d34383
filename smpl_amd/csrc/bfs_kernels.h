// smpl_amd/csrc/bfs_kernels.h -- BFS-3D over brick-major records: k_bfs_init, k_bfs_reset, k_bfs_export, the single-goal
// seed and pass (k_bfs_brick_seed, k_bfs_brick_wave) and the multi-goal ones (k_bfs_brick_seed_multi,
// k_bfs_brick_wave_multi), which share bfs_seed_goal, bfs_visit_brick and bfs_wave_pass.
// Needs nothing from the model or collision headers: device_types.h (SmplxGridDev, SmplxBfsDev, the record layout) and
// bfs_record.h (k_bfs_export reads its cells through bfs_dist) only.
// Restates: bfs3d.cpp:156-201, 507-547; bfs3d.h:213-220; bfs_heuristic.cpp:331-353.
#pragma once

#ifndef __HIPCC_RTC__   // hiprtc (per-robot specialisation, specialize.cpp) brings its own runtime declarations
#include <hip/hip_runtime.h>
#endif

#include "bfs_record.h"
#include "device_types.h"

// ---------------------------------------------------------------------------------------------
// BFS-3D (bfs3d.cpp:156-201 run, 507-547 search), brick formulation over brick-major records (device_types.h
// SmplxBfsDev).  A wave owns an 8x8x8 brick: it loads the brick and its one-cell halo into LDS ONCE, relaxes
// d(c) = min(d(c), min over the 26 neighbours of d + 1) until nothing changes, writes the record back if anything improved,
// and queues the neighbour bricks whose halo it changed.  A pass runs over the queued bricks; passes repeat until none is
// queued.  Hop counts with unit edge costs are the unique fixed point of that relaxation from d(goal) = 0, so the grid equals
// the sequential queue's (bfs3d.cpp:507-547) whatever order bricks are visited in: a brick that read a neighbour's old value
// is queued again by that neighbour when the value drops.  (Round 1 ran one launch per BFS level, 192 at 256^3; round 2 the
// bricks over the reference's x-fastest array.)
// Sentinels as in the reference: WALL 0x7FFFFFFF never changes, UNDISCOVERED -1 stays -1 where no path leads.
// ---------------------------------------------------------------------------------------------
#define SMPLX_BFS_INF 0x7FFFFFFEu
#define SMPLX_BFS_WALLV 0xFFFFFFFEu     // (not 0xFFFFFFFF: a wall + 1 must not wrap to 0 in the branch-free relaxation)
// (SMPLX_BFS_SHARDS, the sub-lists of a pass's brick list, is in device_types.h beside the multi-goal record)

#define SMPLX_BRICK 8
#define SMPLX_BRICK_TILE (SMPLX_BRICK + 2)

// local cell of slot s < SMPLX_BFS_USED of a record (interior, face copy, edge copy, or -- with a coordinate of -1 or 8 -- the
// diagonal neighbour's cell next to a corner)
__device__ __forceinline__ void bfs_slot_cell(int s, int& lx, int& ly, int& lz)
{
    if (s < SMPLX_BFS_FACES) { lz = s >> 6; ly = (s >> 3) & 7; lx = s & 7; return; }
    if (s < SMPLX_BFS_EDGES) {
        const int f = (s - SMPLX_BFS_FACES) >> 6, a = ((s - SMPLX_BFS_FACES) >> 3) & 7, c = (s - SMPLX_BFS_FACES) & 7;
        if (f < 2) { lx = f == 0 ? 0 : 7; lz = a; ly = c; }
        else if (f < 4) { ly = f == 2 ? 0 : 7; lz = a; lx = c; }
        else { lz = f == 4 ? 0 : 7; ly = a; lx = c; }
        return;
    }
    if (s < SMPLX_BFS_CORNERS) {
        const int k = (s - SMPLX_BFS_EDGES) >> 3;
        lz = (s - SMPLX_BFS_EDGES) & 7;
        lx = (k & 1) ? 7 : 0;
        ly = (k & 2) ? 7 : 0;
        return;
    }
    const int c = s - SMPLX_BFS_CORNERS;      // a neighbour's cell, one step outside the brick
    lx = (c & 1) ? 8 : -1;
    ly = (c & 2) ? 8 : -1;
    lz = (c & 4) ? 8 : -1;
}

// every slot of a record that holds cell (lx, ly, lz) takes v
__device__ __forceinline__ void bfs_record_store_cell(int* __restrict__ rec, int lx, int ly, int lz, int v)
{
    rec[(lz << 6) + (ly << 3) + lx] = v;
    if (lx == 0) rec[SMPLX_BFS_FACES + 0 * 64 + lz * 8 + ly] = v;
    if (lx == 7) rec[SMPLX_BFS_FACES + 1 * 64 + lz * 8 + ly] = v;
    if (ly == 0) rec[SMPLX_BFS_FACES + 2 * 64 + lz * 8 + lx] = v;
    if (ly == 7) rec[SMPLX_BFS_FACES + 3 * 64 + lz * 8 + lx] = v;
    if (lz == 0) rec[SMPLX_BFS_FACES + 4 * 64 + ly * 8 + lx] = v;
    if (lz == 7) rec[SMPLX_BFS_FACES + 5 * 64 + ly * 8 + lx] = v;
    if ((lx == 0 || lx == 7) && (ly == 0 || ly == 7)) rec[SMPLX_BFS_EDGES + (((ly == 7) ? 2 : 0) + ((lx == 7) ? 1 : 0)) * 8 + lz] = v;
}

// a CORNER cell of brick (bx, by, bz) also goes into the corner slot of the brick diagonally across it (device_types.h)
__device__ __forceinline__ void bfs_push_corner(int* __restrict__ dist, int bx, int by, int bz, int nbx, int nby, int nbz,
                                                int lx, int ly, int lz, int v)
{
    const int qx = bx + (lx == 7 ? 1 : -1), qy = by + (ly == 7 ? 1 : -1), qz = bz + (lz == 7 ? 1 : -1);
    if (qx < 0 || qy < 0 || qz < 0 || qx >= nbx || qy >= nby || qz >= nbz) return;
    // seen from there this brick lies on the low side of an axis where the cell is at 7
    const int c = (lx == 7 ? 0 : 1) | ((ly == 7 ? 0 : 1) << 1) | ((lz == 7 ? 0 : 1) << 2);
    dist[(size_t)((qz * nby + qy) * nbx + qx) * SMPLX_BFS_REC + SMPLX_BFS_CORNERS + c] = v;
}

// The halo of a brick beyond its six faces: 12 edges of 8 cells and 8 corners, piece e < 104.  Where piece e comes from (the
// neighbour brick (ddx, ddy, ddz), the slot of that brick's record) and where it sits in the 10x10x10 tile: a z-parallel
// edge from the neighbour's edge copies, an x- or y-parallel one from the face copy whose fastest index runs along it, a
// corner from the corner slots of the brick's own record (the diagonal neighbours keep them current: bfs_push_corner).
// Functions of e alone: a lane works them out once per launch.
__device__ __forceinline__ void bfs_edge_piece(int e, int& ddx, int& ddy, int& ddz, int& src, int& pos)
{
    constexpr int TL = SMPLX_BRICK_TILE, TP = SMPLX_BRICK_TILE * SMPLX_BRICK_TILE, HI = SMPLX_BRICK_TILE - 1;
    const int i = e & 7, k = (e >> 3) & 3, g = e >> 5;
    const int s0 = k & 1, s1 = k >> 1;          // 0: the low side (neighbour at -1, its cell 7), 1: the high side
    if (g == 0) {            // z runs; (x, y) sides s0, s1
        ddx = s0 ? 1 : -1; ddy = s1 ? 1 : -1; ddz = 0;
        src = SMPLX_BFS_EDGES + ((s1 ? 0 : 2) + (s0 ? 0 : 1)) * 8 + i;
        pos = (i + 1) * TP + (s1 ? HI : 0) * TL + (s0 ? HI : 0);
    } else if (g == 1) {     // x runs; (y, z) sides s0, s1: the neighbour's y face copy
        ddx = 0; ddy = s0 ? 1 : -1; ddz = s1 ? 1 : -1;
        src = SMPLX_BFS_FACES + (s0 ? 2 : 3) * 64 + (s1 ? 0 : 7) * 8 + i;
        pos = (s1 ? HI : 0) * TP + (s0 ? HI : 0) * TL + (i + 1);
    } else if (g == 2) {     // y runs; (x, z) sides s0, s1: the neighbour's x face copy
        ddx = s0 ? 1 : -1; ddy = 0; ddz = s1 ? 1 : -1;
        src = SMPLX_BFS_FACES + (s0 ? 0 : 1) * 64 + (s1 ? 0 : 7) * 8 + i;
        pos = (s1 ? HI : 0) * TP + (i + 1) * TL + (s0 ? HI : 0);
    } else {                 // corners: e = 96 + (cx | cy << 1 | cz << 2), from the corner slots of the brick's OWN record
        const int cx = i & 1, cy = (i >> 1) & 1, cz = (i >> 2) & 1;
        ddx = 0; ddy = 0; ddz = 0;
        src = SMPLX_BFS_CORNERS + i;
        pos = (cz ? HI : 0) * TP + (cy ? HI : 0) * TL + (cx ? HI : 0);
    }
}

// walls: BfsHeuristic::syncGridAndBfs (bfs_heuristic.cpp:331-353) in integer form:
// wall iff squared cell distance <= wall_thr (largest i with res*sqrt(i) <= radius; -1 if none)
extern "C" __global__ void __launch_bounds__(256)
k_bfs_init(SmplxGridDev g, int wall_thr, int nbx, int nby, int nbz, int* __restrict__ dist)
{
    const size_t total = (size_t)nbx * nby * nbz * SMPLX_BFS_REC;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int s = (int)(i % SMPLX_BFS_REC);
        const size_t b = i / SMPLX_BFS_REC;
        int v = 0x7FFFFFFF;
        if (s < SMPLX_BFS_USED) {
            int lx, ly, lz;
            bfs_slot_cell(s, lx, ly, lz);
            const int cx = (int)(b % nbx) * 8 + lx, cy = (int)(b / nbx % nby) * 8 + ly, cz = (int)(b / ((size_t)nbx * nby)) * 8 + lz;
            if (cx >= 0 && cy >= 0 && cz >= 0 && cx < g.n[0] && cy < g.n[1] && cz < g.n[2]) {      // (a corner slot can lie outside the grid: a wall)
                const size_t brick = ((size_t)(cx >> 2) * g.bricks[1] + (cy >> 2)) * g.bricks[2] + (cz >> 2);
                const int d2 = (int)g.d2[brick * 64 + ((cx & 3) << 4) + ((cy & 3) << 2) + (cz & 3)];
                v = d2 <= wall_thr ? 0x7FFFFFFF : -1;
            }
        }
        dist[i] = v;
    }
}

// BFS_3D::run reset: every non-wall cell back to UNDISCOVERED (bfs3d.cpp:162-166)
extern "C" __global__ void __launch_bounds__(256)
k_bfs_reset(int* __restrict__ dist, size_t total)
{
    for (size_t node = (size_t)blockIdx.x * 256 + threadIdx.x; node < total; node += (size_t)gridDim.x * 256)
        if (dist[node] != 0x7FFFFFFF) dist[node] = -1;
}

// the padded (nx+2)(ny+2)(nz+2) grid in the reference's node order (bfs3d.h:213-220), for smplx_bfs_copy
extern "C" __global__ void __launch_bounds__(256)
k_bfs_export(SmplxBfsDev b, int* __restrict__ out)
{
    const size_t total = (size_t)b.dim_x * b.dim_y * b.dim_z;
    for (size_t node = (size_t)blockIdx.x * 256 + threadIdx.x; node < total; node += (size_t)gridDim.x * 256) {
        const int x = (int)(node % b.dim_x), y = (int)(node / b.dim_x % b.dim_y), z = (int)(node / ((size_t)b.dim_x * b.dim_y));
        int v = 0x7FFFFFFF;
        if (!(x == 0 || x == b.dim_x - 1 || y == 0 || y == b.dim_y - 1 || z == 0 || z == b.dim_z - 1)) {
            const int c[3] = {x - 1, y - 1, z - 1};
            v = bfs_dist(b, c);
        }
        out[node] = v;
    }
}

// The BFS step functions below take their pointers typed as global memory.  A pointer read from a goal's record (the
// multi-goal kernels) is otherwise a generic pointer to the compiler, and every access through it a flat one with its
// address in two VGPRs; for the kernel arguments of the single-goal kernels the cast says what the compiler knows already.
typedef __attribute__((address_space(1))) int bfs_gint;
#define BFS_G(p) ((bfs_gint*)(p))

// the seed of one goal, by one block: its three counter sets cleared, the goal cell labelled 0 and its brick the one entry of
// list 0.  counts: 3 sets x SMPLX_BFS_SHARDS counters, 32 ints apart.  A goal outside the grid (cx < 0) only has its counters
// cleared: nothing is labelled and no pass finds a brick (bfs3d.cpp:169-171)
__device__ __forceinline__ void bfs_seed_goal(bfs_gint* __restrict__ dist, int cx, int cy, int cz, int nbx, int nby, int nbz, bfs_gint* __restrict__ list0,
                                              bfs_gint* __restrict__ counts, int tag_word)
{
    const int t = threadIdx.x;
    if (t < 3 * SMPLX_BFS_SHARDS) counts[32 * t] = 0;
    __syncthreads();
    if (t == 0 && cx >= 0) {
        const int brick = ((cz >> 3) * nby + (cy >> 3)) * nbx + (cx >> 3);
        bfs_record_store_cell((int*)(dist + (size_t)brick * SMPLX_BFS_REC), cx & 7, cy & 7, cz & 7, tag_word);   // distance 0; overwrites a wall at the goal cell, as bfs3d.cpp:178 does
        const int lx = cx & 7, ly = cy & 7, lz = cz & 7;
        if ((lx == 0 || lx == 7) && (ly == 0 || ly == 7) && (lz == 0 || lz == 7)) bfs_push_corner((int*)dist, cx >> 3, cy >> 3, cz >> 3, nbx, nby, nbz, lx, ly, lz, tag_word);
        list0[0] = brick;      // sub-list 0 of list 0
        counts[0] = 1;
    }
}

extern "C" __global__ void __launch_bounds__(64)
k_bfs_brick_seed(int* __restrict__ dist, int cx, int cy, int cz, int nbx, int nby, int nbz, int* __restrict__ list0, int* __restrict__ counts, int tag_word)
{
    if (blockIdx.x == 0) bfs_seed_goal(BFS_G(dist), cx, cy, cz, nbx, nby, nbz, BFS_G(list0), BFS_G(counts), tag_word);
}

// the seeds of all goals of a multi-goal run, one block per goal; block 0 also clears the run's per-pass totals
// (pass_stats: {sum, largest} of the goals' queue sizes for each of n_stats passes)
extern "C" __global__ void __launch_bounds__(64)
k_bfs_brick_seed_multi(const SmplxBfsGoalDev* __restrict__ goals, int nq, int nbx, int nby, int nbz, int* __restrict__ pass_stats, int n_stats)
{
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < 2 * n_stats; i += 64) pass_stats[i] = 0;
    if ((int)blockIdx.x >= nq) return;
    const SmplxBfsGoalDev G = goals[blockIdx.x];
    bfs_seed_goal(BFS_G(G.dist), G.cell[0], G.cell[1], G.cell[2], nbx, nby, nbz, BFS_G(G.lists), BFS_G(G.counts), G.tag_word);
}

// One WAVE per brick (block = 64 lanes): lane (x, y) keeps its z-column of 8 cells in registers: no block barriers, many bricks
// resident per CU, and a change travels the whole column within one sweep (the z direction is relaxed in place, up and
// down), so a brick needs a third of the sweeps of a cell-per-thread version.  In-plane neighbours come from the LDS tile, which
// the lanes refresh with their columns at the start of every sweep; the halo (neighbour bricks' cells) is read once and
// never changes during the sweeps.
// The pass builds the next pass's brick list itself: a neighbour brick is claimed with an atomic exchange on its "queued for the
// next pass" word and appended by the claimer.  Two queued-arrays alternate: a brick clears its own word of the array it was
// queued in, so that array is clean again when it next serves as "next".  Three counter sets rotate (in / next / the one zeroed
// for the pass after).
// Lane shifts of the brick kernel: lane t = ty * 8 + tx holds the z-column at (tx, ty).  A lane outside the brick's 8x8
// contributes SMPLX_BFS_WALLV, which never wins a minimum.
struct BfsLanes { bool has_left, has_right, has_up, has_down; int up_addr, down_addr; };
__device__ __forceinline__ unsigned int bfs_min(unsigned int a, unsigned int b) { return a < b ? a : b; }
// min over the lane and its x neighbours (DPP row_shr:1 / row_shl:1 within the 16-lane row: rows of 8 never straddle one)
__device__ __forceinline__ unsigned int bfs_window_x(const BfsLanes& W, unsigned int x)
{
    const unsigned int l = (unsigned int)__builtin_amdgcn_update_dpp((int)SMPLX_BFS_WALLV, (int)x, 0x111, 0xf, 0xf, false);
    const unsigned int r = (unsigned int)__builtin_amdgcn_update_dpp((int)SMPLX_BFS_WALLV, (int)x, 0x101, 0xf, 0xf, false);
    return bfs_min(x, bfs_min(W.has_left ? l : SMPLX_BFS_WALLV, W.has_right ? r : SMPLX_BFS_WALLV));
}
// min over the lane and its y neighbours (lanes t - 8 and t + 8)
__device__ __forceinline__ unsigned int bfs_window_y(const BfsLanes& W, unsigned int x)
{
    const unsigned int u = (unsigned int)__builtin_amdgcn_ds_bpermute(W.up_addr, (int)x);
    const unsigned int d = (unsigned int)__builtin_amdgcn_ds_bpermute(W.down_addr, (int)x);
    return bfs_min(x, bfs_min(W.has_up ? u : SMPLX_BFS_WALLV, W.has_down ? d : SMPLX_BFS_WALLV));
}

#ifdef SMPLX_BFS_TRACE
// diagnostic build (tools/bfs_trace.sh): every visit leaves the 100 MHz wall clock at its phase boundaries; the longest and
// the sum of each phase over the visits of a pass go to g_bfs_trace[k] / [8 + k], the number of visits to [7]
__device__ long long g_bfs_trace[16];
#define BFS_MARK(k) do { if (t == 0) { const long long now_ = (long long)wall_clock64(); \
    if ((k) > 0) { atomicMax((unsigned long long*)&g_bfs_trace[k], (unsigned long long)(now_ - mark_)); atomicAdd((unsigned long long*)&g_bfs_trace[8 + (k)], (unsigned long long)(now_ - mark_)); } \
    else atomicAdd((unsigned long long*)&g_bfs_trace[7], 1ull); \
    mark_ = now_; } } while (0)
#else
#define BFS_MARK(k) do { } while (0)
#endif

#ifdef SMPLX_BFS_TRACE
#define BFS_TRACE_PARAM , long long& mark_
#define BFS_TRACE_ARG , mark_
#else
#define BFS_TRACE_PARAM
#define BFS_TRACE_ARG
#endif

// the two edge / corner pieces of a lane: pieces t and 64 + t (104 in all); the same for every brick the block visits
struct BfsPieces { int from[2], pos[2]; };

// One visit of brick b by the block's wave, the ONE definition for the single-goal and the multi-goal pass: the load of the
// brick and its halo, the sweeps in registers, the store-back of what improved, the test which neighbours can improve, and
// their claim into the next pass's list (sub-list `shard`).  The caller has taken b from its list and cleared its queued word.
__device__ __forceinline__ void bfs_visit_brick(int b, bfs_gint* __restrict__ dist, int nbx, int nby, int nbz, const BfsPieces& P, unsigned int* tile,
                                                bfs_gint* __restrict__ list_next, bfs_gint* __restrict__ counts_next, int shard_cap, int shard,
                                                bfs_gint* __restrict__ queued_next, int tag_word, int tag_mask BFS_TRACE_PARAM)
{
    constexpr int TL = SMPLX_BRICK_TILE, TP = SMPLX_BRICK_TILE * SMPLX_BRICK_TILE;
    const int t = threadIdx.x;
    const int tx = t & 7, ty = t >> 3;
    const int bxx = b % nbx, byy = (b / nbx) % nby, bzz = b / (nbx * nby);
    unsigned int v[SMPLX_BRICK], before[SMPLX_BRICK];
    {
        // Sixteen loads a lane, all in flight before the first is used and none inside a branch (a load in a branch is
        // waited for before the branches rejoin).  The lane's own column: eight words of the brick's record, 256 bytes
        // apart -- straight to registers.  The halo goes through the tile: six faces, each one 64-word run of a
        // neighbour's face copy; the edges and corners, 104 words, as pieces (bfs_edge_piece).  A neighbour beyond the grid
        // reads as walls.
        const int own = b * SMPLX_BFS_REC;      // (int: up to 2 M bricks)
        int raw[SMPLX_BRICK], face[6], piece[2];
#pragma unroll
        for (int z = 0; z < SMPLX_BRICK; ++z) raw[z] = dist[own + 64 * z + t];
#pragma unroll
        for (int f = 0; f < 6; ++f) {
            const int d = (f & 1) ? 1 : -1;
            const int qx = bxx + (f < 2 ? d : 0), qy = byy + (f >= 2 && f < 4 ? d : 0), qz = bzz + (f >= 4 ? d : 0);
            const bool ok = !(qx < 0 || qy < 0 || qz < 0 || qx >= nbx || qy >= nby || qz >= nbz);      // (uniform)
            const int w = dist[ok ? ((qz * nby + qy) * nbx + qx) * SMPLX_BFS_REC + SMPLX_BFS_FACES + (f ^ 1) * 64 + t : own];
            face[f] = ok ? w : 0x7FFFFFFF;
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int qx = bxx + ((P.from[k] & 3) - 1), qy = byy + (((P.from[k] >> 2) & 3) - 1), qz = bzz + (((P.from[k] >> 4) & 3) - 1);
            const bool ok = !(qx < 0 || qy < 0 || qz < 0 || qx >= nbx || qy >= nby || qz >= nbz);
            const int w = dist[ok ? ((qz * nby + qy) * nbx + qx) * SMPLX_BFS_REC + (P.from[k] >> 6) : own];
            piece[k] = ok ? w : 0x7FFFFFFF;
        }
        auto decode = [&](int w) {
            return w == 0x7FFFFFFF ? SMPLX_BFS_WALLV : ((((w ^ tag_word) & tag_mask) != 0 || w == -1) ? SMPLX_BFS_INF : (unsigned int)(w & ~tag_mask));
        };
#pragma unroll
        for (int z = 0; z < SMPLX_BRICK; ++z) { v[z] = decode(raw[z]); before[z] = v[z]; }
        const int a8 = t >> 3, c8 = t & 7;
#pragma unroll
        for (int f = 0; f < 6; ++f) {
            const int side = (f & 1) ? TL - 1 : 0;
            const int pos = f < 2 ? (a8 + 1) * TP + (c8 + 1) * TL + side : (f < 4 ? (a8 + 1) * TP + side * TL + (c8 + 1) : side * TP + (a8 + 1) * TL + (c8 + 1));
            tile[pos] = decode(face[f]);
        }
        tile[P.pos[0]] = decode(piece[0]);
        if (P.pos[1] >= 0) tile[P.pos[1]] = decode(piece[1]);
    }
    __syncthreads();
    BFS_MARK(2);
    const int col = (ty + 1) * TL + (tx + 1);   // this lane's column in a tile plane
    const bool x_lo = tx == 0, x_hi = tx == SMPLX_BRICK - 1, y_lo = ty == 0, y_hi = ty == SMPLX_BRICK - 1;
    const int xh = x_lo ? 0 : TL - 1, yh = y_lo ? 0 : TL - 1;    // the halo column / row beside a boundary lane
    // in-plane 3x3 minima of the two halo planes, and the least halo cell among the in-plane neighbours of every level of
    // a boundary lane's column: the halo does not change during the visit, so these are read once
    unsigned int p_lo = SMPLX_BFS_WALLV, p_hi = SMPLX_BFS_WALLV;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const unsigned int a = tile[col + dy * TL + dx], c = tile[(TL - 1) * TP + col + dy * TL + dx];
            p_lo = a < p_lo ? a : p_lo;
            p_hi = c < p_hi ? c : p_hi;
        }
    unsigned int halo_min[SMPLX_BRICK];
#pragma unroll
    for (int z = 0; z < SMPLX_BRICK; ++z) halo_min[z] = SMPLX_BFS_WALLV;
    if (x_lo || x_hi) {
#pragma unroll
        for (int z = 0; z < SMPLX_BRICK; ++z)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) halo_min[z] = bfs_min(halo_min[z], tile[(z + 1) * TP + (ty + 1 + dy) * TL + xh]);
    }
    if (y_lo || y_hi) {
#pragma unroll
        for (int z = 0; z < SMPLX_BRICK; ++z)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) halo_min[z] = bfs_min(halo_min[z], tile[(z + 1) * TP + yh * TL + (tx + 1 + dx)]);
    }
    // The sweeps run in registers: the in-plane neighbours of a column are the columns of lanes t -+ 1 (DPP row shifts) and
    // t -+ 8 (ds_bpermute), 3x3 = a row window then a window of row windows.  (Through the LDS tile -- 64 reads, 8 writes and
    // two barriers a sweep -- a sweep took 1.2 us and the nine or so of a brick the front crosses half its visit.)
    const BfsLanes W = {!x_lo, !x_hi, !y_lo, !y_hi, ((t - 8) & 63) << 2, ((t + 8) & 63) << 2};
    bool is_wall[SMPLX_BRICK];
#pragma unroll
    for (int z = 0; z < SMPLX_BRICK; ++z) is_wall[z] = v[z] == SMPLX_BFS_WALLV;
    while (true) {
        // 3x3 in-plane minimum of every level (own cell included): all row windows, then all the shifts of them in flight
        // together, then the halo's share
        unsigned int pm[SMPLX_BRICK], up[SMPLX_BRICK], down[SMPLX_BRICK], start[SMPLX_BRICK];
#pragma unroll
        for (int z = 0; z < SMPLX_BRICK; ++z) { start[z] = v[z]; pm[z] = bfs_window_x(W, v[z]); }
#pragma unroll
        for (int z = 0; z < SMPLX_BRICK; ++z) {
            up[z] = (unsigned int)__builtin_amdgcn_ds_bpermute(W.up_addr, (int)pm[z]);
            down[z] = (unsigned int)__builtin_amdgcn_ds_bpermute(W.down_addr, (int)pm[z]);
        }
#pragma unroll
        for (int z = 0; z < SMPLX_BRICK; ++z)
            pm[z] = bfs_min(bfs_min(pm[z], halo_min[z]), bfs_min(W.has_up ? up[z] : SMPLX_BFS_WALLV, W.has_down ? down[z] : SMPLX_BFS_WALLV));
        // relax the column in place, upwards then downwards: a cell takes 1 + the least of the three plane minima.  No
        // branches (fifteen divergent ones per sweep were most of its time): an undiscovered or wall minimum + 1 stays
        // above every cell value, a wall keeps its own value by a select
#pragma unroll
        for (int z = 0; z < SMPLX_BRICK; ++z) {
            const unsigned int lo = z == 0 ? p_lo : pm[z - 1], hi = z == SMPLX_BRICK - 1 ? p_hi : pm[z + 1];
            const unsigned int nv = bfs_min(v[z], bfs_min(bfs_min(lo, hi), pm[z]) + 1u);
            v[z] = is_wall[z] ? v[z] : nv;
            pm[z] = bfs_min(pm[z], v[z]);
        }
#pragma unroll
        for (int z = SMPLX_BRICK - 2; z >= 0; --z) {
            const unsigned int nv = bfs_min(v[z], pm[z + 1] + 1u);
            v[z] = is_wall[z] ? v[z] : nv;
            pm[z] = bfs_min(pm[z], v[z]);
        }
        unsigned int diff = 0;
#pragma unroll
        for (int z = 0; z < SMPLX_BRICK; ++z) diff |= start[z] ^ v[z];
        if (__ballot(diff != 0u) == 0ull) break;
    }
    BFS_MARK(3);
    // ---- what improved goes back at once, with its face and edge copies (stores are not waited for) ----
    bfs_gint* rec = dist + (size_t)b * SMPLX_BFS_REC;
    bool improved = false;
#pragma unroll
    for (int z = 0; z < SMPLX_BRICK; ++z) {
        if (!(v[z] < before[z])) continue;
        improved = true;
        const int val = (int)v[z] | tag_word;
        rec[(z << 6) + (ty << 3) + tx] = val;
        if (x_lo) rec[SMPLX_BFS_FACES + 0 * 64 + z * 8 + ty] = val;
        if (x_hi) rec[SMPLX_BFS_FACES + 1 * 64 + z * 8 + ty] = val;
        if (y_lo) rec[SMPLX_BFS_FACES + 2 * 64 + z * 8 + tx] = val;
        if (y_hi) rec[SMPLX_BFS_FACES + 3 * 64 + z * 8 + tx] = val;
        if (z == 0) rec[SMPLX_BFS_FACES + 4 * 64 + ty * 8 + tx] = val;
        if (z == SMPLX_BRICK - 1) rec[SMPLX_BFS_FACES + 5 * 64 + ty * 8 + tx] = val;
        if ((x_lo || x_hi) && (y_lo || y_hi)) {
            rec[SMPLX_BFS_EDGES + ((y_hi ? 2 : 0) + (x_hi ? 1 : 0)) * 8 + z] = val;
            if (z == 0 || z == SMPLX_BRICK - 1) bfs_push_corner((int*)dist, bxx, byy, bzz, nbx, nby, nbz, tx, ty, z, val);
        }
    }
    // ---- Which neighbour bricks have to look again: only one that CAN improve -- a cell c' of it (this brick's halo holds
    // its value h as of the load; it can only have become smaller since) next to a cell c of this brick with h > d(c) + 1.
    // (Queueing every neighbour that merely SEES a changed cell made the front revisit the bricks behind and beside it: 2.4
    // visits per brick, most of them a load, one sweep and nothing to write.)  A cell c that did not change in this visit
    // cannot pass the test against a current h (the neighbour was queued when c got its value and has read it since), so
    // "changed" need not be tracked.  A halo cell's neighbours in this brick are a window of the brick's boundary layer
    // -- 3x3 for a face, 3 for an edge, 1 for a corner -- so the test is h against the window minimum, the windows built
    // from the columns by the same lane shifts as the sweeps; the halo values come from the tile (they are as loaded).
    // One bit per direction (oz * 9 + oy * 3 + ox, o = 0 / 1 / 2).
    BFS_MARK(4);
    unsigned int mask = 0;
    if (__ballot(improved) != 0ull) {
        auto can_improve = [](unsigned int h, unsigned int w) { return h != SMPLX_BFS_WALLV && w < SMPLX_BFS_INF && h > w + 1u; };
        const int ox = x_lo ? 0 : 2, oy = y_lo ? 0 : 2;
        const bool on_x = x_lo || x_hi, on_y = y_lo || y_hi;
        unsigned int zw[SMPLX_BRICK];      // window along the column
#pragma unroll
        for (int z = 0; z < SMPLX_BRICK; ++z) {
            zw[z] = v[z];
            if (z > 0) zw[z] = bfs_min(zw[z], v[z - 1]);
            if (z < SMPLX_BRICK - 1) zw[z] = bfs_min(zw[z], v[z + 1]);
        }
        bool fx = false, fy = false, exy = false;
#pragma unroll
        for (int z = 0; z < SMPLX_BRICK; ++z) {
            const unsigned int yz = bfs_window_y(W, zw[z]), xz = bfs_window_x(W, zw[z]);   // (every lane takes part in the shifts)
            const unsigned int hx = tile[(z + 1) * TP + (ty + 1) * TL + xh], hy = tile[(z + 1) * TP + yh * TL + (tx + 1)];
            const unsigned int hxy = tile[(z + 1) * TP + yh * TL + xh];
            fx = fx || can_improve(hx, yz);
            fy = fy || can_improve(hy, xz);
            exy = exy || can_improve(hxy, zw[z]);
        }
        if (on_x && fx) mask |= 1u << (1 * 9 + 1 * 3 + ox);
        if (on_y && fy) mask |= 1u << (1 * 9 + oy * 3 + 1);
        if (on_x && on_y && exy) mask |= 1u << (1 * 9 + oy * 3 + ox);
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const unsigned int vz = side == 0 ? v[0] : v[SMPLX_BRICK - 1];
            const int zs = side == 0 ? 0 : TL - 1, oz = side == 0 ? 0 : 2;
            const unsigned int xw = bfs_window_x(W, vz), yw = bfs_window_y(W, vz), xy = bfs_window_y(W, xw);
            if (can_improve(tile[zs * TP + col], xy)) mask |= 1u << (oz * 9 + 1 * 3 + 1);
            if (on_x && can_improve(tile[zs * TP + (ty + 1) * TL + xh], yw)) mask |= 1u << (oz * 9 + 1 * 3 + ox);
            if (on_y && can_improve(tile[zs * TP + yh * TL + (tx + 1)], xw)) mask |= 1u << (oz * 9 + oy * 3 + 1);
            if (on_x && on_y && can_improve(tile[zs * TP + yh * TL + xh], vz)) mask |= 1u << (oz * 9 + oy * 3 + ox);
        }
    }
    BFS_MARK(5);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mask |= (unsigned int)__shfl_xor((int)mask, off);
    int claimed = -1;
    if (t < 27 && t != 13 && ((mask >> t) & 1u)) {
        const int qx = bxx + t % 3 - 1, qy = byy + (t / 3) % 3 - 1, qz = bzz + t / 9 - 1;
        if (!(qx < 0 || qy < 0 || qz < 0 || qx >= nbx || qy >= nby || qz >= nbz)) {
            const int q = (qz * nby + qy) * nbx + qx;
            if (atomicExch((int*)&queued_next[q], 1) == 0) claimed = q;
        }
    }
    const unsigned long long cm = __ballot(claimed >= 0);
    if (cm != 0) {
                int base = 0;
        if (t == 0) base = atomicAdd((int*)&counts_next[32 * shard], __popcll(cm));
        base = __shfl(base, 0);
        if (claimed >= 0) {
            const int pos = base + __popcll(cm & ((1ull << t) - 1ull));
            if (pos < shard_cap) list_next[(size_t)shard * shard_cap + pos] = claimed;
        }
    }
    BFS_MARK(6);
    __syncthreads();   // the tile is reused by the block's next brick
}

// One pass over one goal's queued bricks by the blocks [0, nblocks) of a launch, `block` being this one: the list is the
// SMPLX_BFS_SHARDS sub-lists of list_in, block strides over it.  The goal's first block clears the counters of the pass after
// the next and leaves the queue size in queue_size_out (if not null).  Returns the queue size.
__device__ __forceinline__ int bfs_wave_pass(int block, int nblocks, bfs_gint* __restrict__ dist, int nbx, int nby, int nbz,
                                             const bfs_gint* __restrict__ list_in, const bfs_gint* __restrict__ counts_in, bfs_gint* __restrict__ list_next,
                                             bfs_gint* __restrict__ counts_next, bfs_gint* __restrict__ counts_after, int shard_cap,
                                             bfs_gint* __restrict__ queued_mine, bfs_gint* __restrict__ queued_next, bfs_gint* __restrict__ queue_size_out,
                                             int tag_word, int tag_mask, unsigned int* tile)
{
    int pre[SMPLX_BFS_SHARDS + 1];
    pre[0] = 0;
#pragma unroll
    for (int k = 0; k < SMPLX_BFS_SHARDS; ++k) pre[k + 1] = pre[k] + counts_in[32 * k];
    const int n = pre[SMPLX_BFS_SHARDS];
    const int t = threadIdx.x;
    if (block == 0 && t < SMPLX_BFS_SHARDS) counts_after[32 * t] = 0;
    if (block == 0 && t == 0 && queue_size_out) *queue_size_out = n;   // the host sizes the next goal's launches by it
    BfsPieces P;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        int ddx, ddy, ddz, src, pos;
        bfs_edge_piece(t + 64 * k < 104 ? t + 64 * k : 0, ddx, ddy, ddz, src, pos);
        P.from[k] = (ddx + 1) | ((ddy + 1) << 2) | ((ddz + 1) << 4) | (src << 6);
        P.pos[k] = t + 64 * k < 104 ? pos : -1;
    }
#ifdef SMPLX_BFS_TRACE
    long long mark_ = 0;
#endif
    for (int it = block; it < n; it += nblocks) {
        int sh = 0;
#pragma unroll
        for (int k = 1; k < SMPLX_BFS_SHARDS; ++k) sh += it >= pre[k] ? 1 : 0;
        BFS_MARK(0);
        const int b = list_in[(size_t)sh * shard_cap + (it - pre[sh])];
        if (t == 0) queued_mine[b] = 0;
        BFS_MARK(1);
        bfs_visit_brick(b, dist, nbx, nby, nbz, P, tile, list_next, counts_next, shard_cap, block % SMPLX_BFS_SHARDS, queued_next, tag_word, tag_mask BFS_TRACE_ARG);
    }
    return n;
}

extern "C" __global__ void __launch_bounds__(64)
k_bfs_brick_wave(int* __restrict__ dist, int nbx, int nby, int nbz,
                 const int* __restrict__ list_in, const int* __restrict__ counts_in, int* __restrict__ list_next,
                 int* __restrict__ counts_next, int* __restrict__ counts_after, int shard_cap,
                 int* __restrict__ queued_mine, int* __restrict__ queued_next, int* __restrict__ queue_size_out, int tag_word, int tag_mask)
{
    __shared__ unsigned int tile[SMPLX_BRICK_TILE * SMPLX_BRICK_TILE * SMPLX_BRICK_TILE];
    (void)bfs_wave_pass((int)blockIdx.x, (int)gridDim.x, BFS_G(dist), nbx, nby, nbz, BFS_G(list_in), BFS_G(counts_in), BFS_G(list_next), BFS_G(counts_next),
                        BFS_G(counts_after), shard_cap, BFS_G(queued_mine), BFS_G(queued_next), BFS_G(queue_size_out), tag_word, tag_mask, tile);
}

// Pass `pass` of a multi-goal run: blockIdx.y is the goal, blockIdx.x strides over that goal's list exactly as in the
// single-goal pass, with the lists, counters, queued words and tag of the goal's own record -- the goals share launches
// and nothing else, so each goal's records go through the same label-correcting sweep to the same fixed point.  A block
// whose goal has nothing queued reads its counters and leaves.  The two lists and queued arrays alternate and the three
// counter sets rotate by `pass` as in run_bfs.  Each goal's first block adds its queue size to stats[0] and raises stats[1] to
// it (stats: this pass's slot, null = not kept): the host learns from one word whether any goal has a brick queued.
// history_slot: where behind the counters the goal's queue size goes, -1 = nowhere.
extern "C" __global__ void __launch_bounds__(64)
k_bfs_brick_wave_multi(const SmplxBfsGoalDev* __restrict__ goals, int nbx, int nby, int nbz, int pass, int history_slot, int* __restrict__ stats)
{
    __shared__ unsigned int tile[SMPLX_BRICK_TILE * SMPLX_BRICK_TILE * SMPLX_BRICK_TILE];
    const SmplxBfsGoalDev G = goals[blockIdx.y];
    if (G.cell[0] < 0) return;     // outside the grid: nothing is labelled (bfs3d.cpp:169-171)
    const int nbricks = nbx * nby * nbz;
    const size_t list_ints = (size_t)SMPLX_BFS_SHARDS * nbricks, set_ints = (size_t)SMPLX_BFS_SHARDS * 32;
    const int in = pass & 1, out = (pass + 1) & 1;
    bfs_gint* const dist = BFS_G(G.dist);
    bfs_gint* const lists = BFS_G(G.lists);
    bfs_gint* const counts = BFS_G(G.counts);
    bfs_gint* const queued = BFS_G(G.queued);
    const int n = bfs_wave_pass((int)blockIdx.x, (int)gridDim.x, dist, nbx, nby, nbz, lists + in * list_ints, counts + (pass % 3) * set_ints,
                                lists + out * list_ints, counts + ((pass + 1) % 3) * set_ints, counts + ((pass + 2) % 3) * set_ints, nbricks,
                                queued + (size_t)in * nbricks, queued + (size_t)out * nbricks,
                                history_slot >= 0 ? counts + SMPLX_BFS_COUNTERS + history_slot : (bfs_gint*)nullptr, G.tag_word, G.tag_mask, tile);
    if (blockIdx.x == 0 && threadIdx.x == 0 && stats && n > 0) { atomicAdd(&stats[0], n); atomicMax(&stats[1], n); }
}
