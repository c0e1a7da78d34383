// smpl_amd/csrc/search_table.h -- the state table as the workgroup of a device-resident search reads and writes it.
// Owns: coord_hash_lds, TableProbe with table_probe_start / table_probe_finish, table_store_own, k_search_table_fill and
// the parity-test kernel k_table_probe_ops.  The slot's loader and its compare (table_slot_load, table_slot_match,
// SMPLX_TABLE_WORDS) are shared with the step kernels: lattice_steps.h.  search_kernel.h builds getOrCreateState from them.
// Restates: manip_lattice.cpp:1302-1354 (getHashEntry, createHashEntry).
#pragma once

#include "lattice_steps.h"

__device__ __forceinline__ unsigned int coord_hash_lds(const LDS_AS int* c, int n)
{
    unsigned int h = 2166136261u;
    for (int i = 0; i < n; ++i) h = (h ^ (unsigned int)c[i]) * 16777619u;
    h ^= h >> 15; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

// One probe sequence of the state table with plain 16-byte loads.  Only the workgroup that owns the query writes its table
// while the kernel runs, so what it reads is current.  table_probe_start issues the loads of the home slot (the caller
// puts the planning-link FK between the two, for the loads to travel behind); table_probe_finish looks at them and walks on
// if it has to.
struct TableProbe { int id; unsigned int free_slot; };
typedef TableSlotWords TableProbeLoads;
__device__ __forceinline__ TableProbeLoads table_probe_start(const SmplxTableDev& T, int nv, unsigned int hash)
{
    TableProbeLoads r;
    r.slot = hash & T.mask;
    table_slot_load(T, r.slot, nv, r.w);
    return r;
}
__device__ __forceinline__ TableProbe table_probe_finish(const SmplxTableDev& T, TableProbeLoads& ld, const LDS_AS int* c, int nv)
{
    TableProbe r;
    while (true) {
        if (ld.w[0].x == 0) { r.id = -1; r.free_slot = ld.slot; return r; }
        if (ld.w[0].x > 0 && table_slot_match(ld.w, c, nv)) { r.id = ld.w[0].x - 1; r.free_slot = 0; return r; }
        ld.slot = (ld.slot + 1) & T.mask;
        table_slot_load(T, ld.slot, nv, ld.w);
    }
}
__device__ __forceinline__ void table_store_own(const SmplxTableDev& T, unsigned int slot, const LDS_AS int* c, int nv, int id)
{
    SMPLX_GLOBAL_AS int* sl = as_global(T.slots) + (size_t)slot * T.stride;
    for (int v = 0; v < nv; ++v) sl[1 + v] = c[v];
    sl[0] = id + 1;
}

// getOrCreateState for states the device table does not hold yet (the start state the host created; every state after
// the table was enlarged): inserts ids [first, n) of the query's coordinate array
extern "C" __global__ void __launch_bounds__(256)
k_search_table_fill(const SmplxSpaceDev* __restrict__ Sq, const int* __restrict__ coord, int first, int n, int nvars)
{
    const SmplxTableDev T = Sq->table;
    for (int id = first + blockIdx.x * blockDim.x + threadIdx.x; id < n; id += gridDim.x * blockDim.x) {
        if (id == 0) continue;      // the goal id has no coordinate (manip_lattice.cpp:122)
        const int* c = coord + (size_t)id * nvars;
        unsigned int k = smplx_coord_hash(c, nvars) & T.mask;
        while (true) {
            SMPLX_GLOBAL_AS int* sl = as_global(T.slots) + (size_t)k * T.stride;
            if (atomicCAS((int*)&sl[0], 0, -(id + 1)) == 0) {
                for (int v = 0; v < nvars; ++v) sl[1 + v] = c[v];
                __threadfence();
                __atomic_store_n(&sl[0], id + 1, __ATOMIC_RELAXED);
                break;
            }
            k = (k + 1) & T.mask;
        }
    }
}

// Parity-test kernel (test_hooks.h): the state-table probe of k_search (table_probe_start / table_probe_finish /
// table_store_own) on a table of the caller's size.  insert = 1: one lane takes the n coordinates in turn, probes, and stores
// coordinate i under id i where the probe found none (out[i] = what the probe found, -1 for a new coordinate); insert = 0:
// every lane looks its share of the n coordinates up (out[i] = id or -1).  one_home: every coordinate's probe starts at
// slot 0 instead of its hash, so that a lookup walks over every state inserted before the one it looks for.
extern "C" __global__ void __launch_bounds__(64)
k_table_probe_ops(SmplxTableDev T, const int* __restrict__ coords, int n, int nv, int one_home, int insert, int* __restrict__ out)
{
    __shared__ int cbuf[64][SMPLX_MAX_VARS];
    const int lane = threadIdx.x;
    if (insert && lane != 0) return;
    for (int i = lane; i < n; i += insert ? 1 : 64) {
        for (int v = 0; v < nv; ++v) cbuf[lane][v] = coords[(size_t)i * nv + v];
        const LDS_AS int* c = (const LDS_AS int*)cbuf[lane];
        const unsigned int hash = one_home ? 0u : coord_hash_lds(c, nv);
        TableProbeLoads ld = table_probe_start(T, nv, hash);
        const TableProbe pr = table_probe_finish(T, ld, c, nv);
        out[i] = pr.id;
        if (insert && pr.id < 0) {
            table_store_own(T, pr.free_slot, c, nv, i);
            __threadfence();
        }
    }
}
