// smpl_amd/csrc/vox_common.h -- what the voxelisers of field.hip share (mesh_voxelizer.h, octree_voxelizer.h,
// object_sphere_rows.h): the lists a run returns, the block-rank step of an ordered compaction, the timer of the test
// hook, and an exclusive scan on the device.  Stands behind no line of the reference of its own: the orders it keeps
// are those of smpl/src/geometry/voxelize.cpp:1008-1035 (cells in mask order) and
// sbpl_collision_checking/src/voxel_operations.cpp:405-436 (octree points in generation order).
#pragma once

namespace {

// the cell lists of one run, the shapes' lists back to back
struct VoxLists {
    DevPtr<int32_t> d_cells;          // n x 3, on the device
    std::vector<int> first, box;      // as in WorldObject
};

// one step of an ordered compaction over a block: of the threads with `on`, how many sit in the wavefronts before this
// one (before), how many in this one's lower lanes (rank), how many in the block (all).  wave_n: FIELD_BLOCK / 64 ints
// of LDS; a caller that takes another step puts a barrier between them.
struct BlockRank { int before, rank, all; };
__device__ __forceinline__ BlockRank block_rank(bool on, int* wave_n)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(on);
    if (lane == 0) wave_n[wave] = __popcll(b);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < FIELD_BLOCK / 64; ++w) { before += w < wave ? wave_n[w] : 0; all += wave_n[w]; }
    return BlockRank{before, (int)__popcll(b & ((1ull << lane) - 1ull)), all};
}

// test hook (tools/voxelize_time.py): when on, the voxelisers bracket their launches with events
bool g_vox_timing = false;
double g_vox_kernel_ms = 0.0;

// with the test hook on, the time between begin() and end() is added to g_vox_kernel_ms; end() also reports launch errors
struct VoxTimer {
    DevEvent a, b;
    hipError_t begin()
    {
        if (!g_vox_timing) return hipSuccess;
        if (!a) { if (hipError_t e = a.create()) return e; if (hipError_t e = b.create()) return e; }
        return hipEventRecord(a, 0);
    }
    hipError_t end()
    {
        if (hipError_t e = hipGetLastError()) return e;
        if (!g_vox_timing) return hipSuccess;
        if (hipError_t e = hipEventRecord(b, 0)) return e;
        if (hipError_t e = hipEventSynchronize(b)) return e;
        float ms = 0.f;
        if (hipError_t e = hipEventElapsedTime(&ms, a, b)) return e;
        g_vox_kernel_ms += (double)ms;
        return hipSuccess;
    }
};

// exclusive scan, in place, of every tile of FIELD_BLOCK entries of v; sums[tile] = the tile's total.  With trips the
// entries are not read but made: entry i < n - 1 is the points of leaf i, the product of its trips, and entry n - 1 is 0
// (the scan turns it into the total).
__global__ void __launch_bounds__(FIELD_BLOCK)
k_scan_tiles(long long* __restrict__ v, int n, long long* __restrict__ sums, const int* __restrict__ trips)
{
    __shared__ long long s[2][FIELD_BLOCK];
    const int i = blockIdx.x * FIELD_BLOCK + threadIdx.x;
    long long own = 0;
    if (trips) { if (i < n - 1) own = (long long)trips[3 * (size_t)i] * trips[3 * (size_t)i + 1] * trips[3 * (size_t)i + 2]; }
    else if (i < n) own = v[i];
    int cur = 0;
    s[0][threadIdx.x] = own;
    __syncthreads();
    for (int d = 1; d < FIELD_BLOCK; d <<= 1) {          // Hillis-Steele: after the step with d, s holds sums of 2d entries
        s[cur ^ 1][threadIdx.x] = s[cur][threadIdx.x] + ((int)threadIdx.x >= d ? s[cur][threadIdx.x - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    if (i < n) v[i] = s[cur][threadIdx.x] - own;
    if (threadIdx.x == FIELD_BLOCK - 1) sums[blockIdx.x] = s[cur][threadIdx.x];
}

// adds the scanned tile totals back: v[i] += sums[tile of i]
__global__ void __launch_bounds__(FIELD_BLOCK)
k_scan_add(long long* __restrict__ v, int n, const long long* __restrict__ sums)
{
    const int i = blockIdx.x * FIELD_BLOCK + threadIdx.x;
    if (i < n) v[i] += sums[blockIdx.x];
}

// entries of scratch an exclusive scan of n entries needs: the tile totals of every level
size_t scan_scratch(size_t n)
{
    size_t total = 0;
    do { n = (n + FIELD_BLOCK - 1) / FIELD_BLOCK; total += n; } while (n > 1);
    return total;
}

// exclusive scan of v[0 .. n) in place on the device: tiles of FIELD_BLOCK, their totals scanned the same way, added back.
// With trips, v is first filled with the leaves' points (k_scan_tiles).
void scan_exclusive(long long* v, int n, long long* scratch, const int* trips = nullptr)
{
    const int tiles = (n + FIELD_BLOCK - 1) / FIELD_BLOCK;
    hipLaunchKernelGGL(k_scan_tiles, dim3(tiles), dim3(FIELD_BLOCK), 0, 0, v, n, scratch, trips);
    if (tiles == 1) return;
    scan_exclusive(scratch, tiles, scratch + tiles);
    hipLaunchKernelGGL(k_scan_add, dim3(tiles), dim3(FIELD_BLOCK), 0, 0, v, n, (const long long*)scratch);
}

}  // namespace
