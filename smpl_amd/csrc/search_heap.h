// smpl_amd/csrc/search_heap.h -- OPEN of the device-resident ARA*: the reference's binary heap, worked by one wave.
// Owns: SearchLds (what the waves of a k_search block share; the ancestor cache in it is the heap's), hent_t, HeapRef with
// hget / hput / hset, the sequential sift and the level-parallel make (heap_percolate_down, heap_make_block), the wave
// helpers (wave_rl*), the wave-parallel sifts (heap_sift_up_wave, heap_sift_down_wave), heap_pop_wave,
// heap_refresh_duplicates_wave, the ancestor cache (ancestor_cache_fill, ac_update, hset_ac), search_key and
// heap_rekey_block, and the parity-test kernel k_heap_ops.  search_kernel.h builds k_search from them.
// Restates: smpl/include/smpl/detail/intrusive_heap.hpp:145-166 (push / pop), 197-213 (erase, make), 346-395 (the sift
// rules: strict '<', the left child only if left < right); arastar.cpp:571-582 (reorderOpen, computeKey).
//
// The sifts are wave-parallel and exact: sift-up reads ALL ancestors of the slot at once (lane j: index >> j), a ballot
// finds the level the sequential loop would stop at, the ancestors below it move down in one scatter; sift-down fetches
// the five levels under the pivot at once (62 lanes) and resolves the path in registers.
// The first `lh` entries of the heap array live in LDS while k_search runs, the rest in HBM; the HBM-resident ancestors of
// the slots a relaxation's pushes will take are fetched into LDS in one round trip before it (written through by every sift).
#pragma once

#include "model_lds.h"     // LDS_AS, as_global

#define SMPLX_AC_LEVELS 16
#define SMPLX_AC_SLOTS 128

// what the waves of the block share
struct SearchLds {
    int action;                            // the round, published before its first barrier
    int buf;                               // ... and the ExpandLds it works on
    int seq;                               // ... and its number
    int helper_gave_up;                    // the helper wave's wait for `go` ran out (never seen; turns into SMPLX_SS_ERROR)
    int go;                                // = seq once the state table holds everything committed before this round's state was
                                           //   popped: the helper wave may probe it (the search wave sets it before it joins the round's end)
    double reorder_eps;
    int reorder_size, reorder_dups;
    // ancestors of the slots the pushes of a relaxation will take, as far as they lie in HBM: level j (1 = parents) holds
    // heap indices ac_lo[j] .. ac_hi[j] at ac_val[ac_base[j] ...]
    int ac_nlev;
    int ac_lo[SMPLX_AC_LEVELS + 1], ac_hi[SMPLX_AC_LEVELS + 1], ac_base[SMPLX_AC_LEVELS + 1];
    unsigned long long ac_val[SMPLX_AC_SLOTS];
};

// a heap entry as one 64-bit word (the layout of SmplxHeapEntry: f in the low half, id in the high half): LDS and HBM
// copies are single loads / stores
typedef unsigned long long hent_t;
#define HENT_ABSENT (~0ull)
__device__ __forceinline__ unsigned int hent_f(hent_t e) { return (unsigned int)e; }
__device__ __forceinline__ int hent_id(hent_t e) { return (int)(e >> 32); }
__device__ __forceinline__ hent_t hent_make(unsigned int f, int id) { return (hent_t)f | ((hent_t)(unsigned int)id << 32); }

struct HeapRef {
    LDS_AS hent_t* lds;                    // entries [0, lh)
    SMPLX_GLOBAL_AS hent_t* hbm;           // entries [lh, ...)
    SMPLX_GLOBAL_AS SmplxSState* st;
    int lh;
};

__device__ __forceinline__ hent_t hget(const HeapRef& H, int i)
{
    if (i < H.lh) return H.lds[i];
    return H.hbm[i];
}
// the entry alone (the state's heap_index is not touched)
__device__ __forceinline__ void hput(const HeapRef& H, int i, hent_t e)
{
    if (i < H.lh) H.lds[i] = e;
    else H.hbm[i] = e;
}
// place an entry and record its position in the state (intrusive_heap.hpp: m_data[i] = e; e->m_heap_index = i)
__device__ __forceinline__ void hset(const HeapRef& H, int i, hent_t e)
{
    hput(H, i, e);
    H.st[hent_id(e)].heap_index = i;
}

// ---- the sequential forms (one thread): the reference's loops as they stand.  Used by the level-parallel make() and as the
// specification of the wave-parallel forms below ----

// intrusive_heap.hpp:346-377; size = number of elements (the reference's m_data.size() - 1)
__device__ __forceinline__ void heap_percolate_down(const HeapRef& H, int pivot, int size)
{
    if (pivot > size) return;
    int left = pivot << 1, right = left + 1;
    const hent_t tmp = hget(H, pivot);
    while (left <= size) {
        hent_t es = hget(H, left);
        int s = left;
        if (right <= size) {
            const hent_t er = hget(H, right);
            if (!(hent_f(es) < hent_f(er))) { es = er; s = right; }
        }
        if (hent_f(es) < hent_f(tmp)) {
            hset(H, pivot, es);
            pivot = s;
        } else break;
        left = pivot << 1; right = left + 1;
    }
    hset(H, pivot, tmp);
}

// intrusive_heap.hpp:208-213 make(): percolate_down(i) for i = size/2 .. 1, by ALL threads of the block.  Nodes of one depth
// own disjoint subtrees, so a depth is sifted by all threads at once, deepest first -- the result is the sequential
// loop's.  With the same element twice in the array (`duplicates`) two sifts could race on its heap_index: then thread 0
// runs the loop alone.  Ends with a barrier.
__device__ __forceinline__ void heap_make_block(const HeapRef& H, int size, bool duplicates)
{
    const int t = threadIdx.x;
    if (duplicates) {
        if (t == 0) for (int i = size >> 1; i >= 1; --i) heap_percolate_down(H, i, size);
        __syncthreads();
        return;
    }
    int top_depth = 0;
    while ((2 << top_depth) <= (size >> 1)) ++top_depth;      // depth of node size/2
    for (int d = top_depth; d >= 0; --d) {
        const int first = 1 << d;
        int lastn = (2 << d) - 1;
        if (lastn > (size >> 1)) lastn = size >> 1;
        for (int i = first + t; i <= lastn; i += blockDim.x) heap_percolate_down(H, i, size);
        __syncthreads();
    }
}

// ARAStar::computeKey (arastar.cpp:579-582)
__device__ __forceinline__ unsigned int search_key(double eps, unsigned int g, unsigned int h)
{
    return g + (unsigned int)(long long)(eps * (double)h);
}

// ARAStar::reorderOpen (arastar.cpp:571-577) by ALL threads of the block: f of every OPEN entry under the new epsilon, in
// the state and in the entry, then make().  Precondition: st == H.st (the caller hands over the pointer it has at hand, so
// that this loop does not keep H.st alive beside it).  It contains block barriers -- one between the two passes and those
// of heap_make_block -- so every thread of the block runs this loop and these barriers at the same moment, with the same
// size, eps and duplicates.
__device__ __forceinline__ void heap_rekey_block(const HeapRef& H, SMPLX_GLOBAL_AS SmplxSState* st, int size, double eps, bool duplicates)
{
    for (int i = 1 + (int)threadIdx.x; i <= size; i += blockDim.x) {
        const int eid = hent_id(hget(H, i));
        SMPLX_GLOBAL_AS SmplxSState* ss = &st[eid];
        const unsigned int f = search_key(eps, ss->g, ss->h);
        ss->f = f;
        hput(H, i, hent_make(f, eid));
    }
    __syncthreads();
    heap_make_block(H, size, duplicates);
}

// ---- wave-level helpers: every lane of the wave is active and `lane_index` arguments are uniform ----
__device__ __forceinline__ int wave_rl(int v, int lane_index) { return __builtin_amdgcn_readlane(v, lane_index); }
__device__ __forceinline__ unsigned int wave_rlu(unsigned int v, int lane_index) { return (unsigned int)__builtin_amdgcn_readlane((int)v, lane_index); }
__device__ __forceinline__ hent_t wave_rl64(hent_t v, int lane_index)
{
    const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)v, lane_index);
    const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(v >> 32), lane_index);
    return (hent_t)lo | ((hent_t)hi << 32);
}
__device__ __forceinline__ double wave_rl_f64(double v, int lane_index)
{
    return __longlong_as_double((long long)wave_rl64((unsigned long long)__double_as_longlong(v), lane_index));
}

// a write to the HBM part of the heap also refreshes the ancestor cache where it holds that index
__device__ __forceinline__ void ac_update(SearchLds& W, int i, hent_t e)
{
    const int nlev = W.ac_nlev;
    for (int j = 1; j <= nlev; ++j)
        if (i >= W.ac_lo[j] && i <= W.ac_hi[j]) { W.ac_val[W.ac_base[j] + i - W.ac_lo[j]] = e; return; }
}
__device__ __forceinline__ void hset_ac(const HeapRef& H, SearchLds& W, int i, hent_t e)
{
    if (i < H.lh) H.lds[i] = e;
    else { H.hbm[i] = e; ac_update(W, i, e); }
    H.st[hent_id(e)].heap_index = i;
}

// percolate_up by the whole wave (intrusive_heap.hpp:379-395): entry e sifts up from slot `start` (a push: the new last slot;
// decrease: the entry's slot).  Lane j reads the ancestor start >> j; the sequential loop compares every ancestor IN ITS
// ORIGINAL PLACE with e and stops at the first that is smaller, so a ballot finds that level; the ancestors below it move
// down one level each, e takes the freed slot.  `cached` = the ancestor cache covers the walk (a push of the relaxation it
// was built for): HBM-resident ancestors are read from LDS.
__device__ __forceinline__ void heap_sift_up_wave(const HeapRef& H, SearchLds& W, int lane, int start, hent_t e, bool cached)
{
    const int j = lane;
    const int idx = j < 31 ? (start >> j) : 0;
    const bool anc = j >= 1 && idx >= 1;
    hent_t ent = 0;
    if (anc) {
        if (idx < H.lh) ent = H.lds[idx];
        else if (cached && j <= W.ac_nlev && idx >= W.ac_lo[j] && idx <= W.ac_hi[j]) ent = W.ac_val[W.ac_base[j] + idx - W.ac_lo[j]];
        else ent = H.hbm[idx];
    }
    const unsigned long long m_anc = __ballot(anc), m_stop = __ballot(anc && hent_f(ent) < hent_f(e));
    const int jstop = m_stop ? __ffsll((long long)m_stop) - 1 : __popcll(m_anc) + 1;   // ancestors are lanes 1 .. popc(m_anc)
    if (!cached) {
        if (anc && j < jstop) hset_ac(H, W, start >> (j - 1), ent);
        if (j == 0) hset_ac(H, W, start >> (jstop - 1), e);
        return;
    }
    // a walk the cache was built for: a write to level l of the walk can only concern the cache's level l (level 0, the new
    // slots themselves, is not cached)
    const bool mover = anc && j < jstop;
    if (mover || j == 0) {
        const int l = mover ? j - 1 : jstop - 1;
        const int dst = start >> l;
        const hent_t v = mover ? ent : e;
        if (dst < H.lh) H.lds[dst] = v;
        else {
            H.hbm[dst] = v;
            if (l >= 1 && l <= W.ac_nlev && dst >= W.ac_lo[l] && dst <= W.ac_hi[l]) W.ac_val[W.ac_base[l] + dst - W.ac_lo[l]] = v;
        }
        H.st[hent_id(v)].heap_index = dst;
    }
}

// percolate_down by the whole wave (intrusive_heap.hpp:346-377): entry tmp sifts down from `pivot`.  Lanes 0 .. 61 fetch the
// five levels under the pivot at once; the path is resolved in registers (the loop reads every child in its original place:
// moves only ever write to slots ABOVE what is read next); the chosen entries move up in one scatter.
__device__ __forceinline__ void heap_sift_down_wave(const HeapRef& H, int lane, int pivot, int size, hent_t tmp)
{
    const int lv = 31 - __clz(lane + 2);                    // level below the pivot: 1 .. 5 for lanes 0 .. 61
    const int off = lane + 2 - (1 << lv);
    while (true) {
        if ((pivot << 1) > size) break;
        const int idx = (pivot << lv) + off;
        hent_t ent = HENT_ABSENT;
        if (lane < 62 && idx <= size) ent = hget(H, idx);
        int c = 0, depth = 0;
        unsigned long long chosen = 0;
        bool stopped = false;
#pragma unroll
        for (int l = 1; l <= 5; ++l) {
            if (stopped) continue;
            const int li = (1 << l) - 2 + 2 * c;
            const hent_t el = wave_rl64(ent, li), er = wave_rl64(ent, li + 1);
            if (el == HENT_ABSENT) { stopped = true; continue; }
            const bool right = er != HENT_ABSENT && !(hent_f(el) < hent_f(er));
            const hent_t es = right ? er : el;
            if (!(hent_f(es) < hent_f(tmp))) { stopped = true; continue; }
            chosen |= 1ull << (li + (right ? 1 : 0));
            c = 2 * c + (right ? 1 : 0);
            depth = l;
        }
        if ((chosen >> lane) & 1ull) hset(H, idx >> 1, ent);
        pivot = (pivot << depth) + c;
        if (stopped) break;
        // the next round reads below what this one moved: nothing it reads was written
    }
    if (lane == 0) hset(H, pivot, tmp);
}

// pop by the whole wave (intrusive_heap.hpp:155-166): the top, state `top_id`, leaves OPEN and the last entry sifts down
// from the root.  `last` = the entry of slot `size`, which the caller loads together with whatever else it needs of the
// popped state, behind a fence that orders the loads with the wave's earlier stores; `size` comes back one smaller.
__device__ __forceinline__ void heap_pop_wave(const HeapRef& H, int lane, int top_id, int& size, hent_t last)
{
    if (lane == 0) H.st[top_id].heap_index = 0;
    --size;
    if (size >= 1) heap_sift_down_wave(H, lane, 1, size, last);
}

// Every OPEN entry of state `id` takes the state's new f (whole wave).  Only needed once a state has been pushed while
// already in OPEN (the reference appends a state to INCONS once per improvement, arastar.cpp:563-565, and pushes every
// INCONS entry, :180-184): its heap then holds the same element twice, and both see an f change because both point to it.
__device__ __forceinline__ void heap_refresh_duplicates_wave(const HeapRef& H, SearchLds& W, int lane, int size, int id, unsigned int f)
{
    for (int i = 1 + lane; i <= size; i += 64) {
        const hent_t e = hget(H, i);
        if (hent_id(e) == id && hent_f(e) != f) {
            const hent_t ne = hent_make(f, id);
            if (i < H.lh) H.lds[i] = ne; else { H.hbm[i] = ne; ac_update(W, i, ne); }
        }
    }
}

// Ancestors of the slots n + 1 .. n + cnt (where a relaxation's pushes go) that lie beyond the LDS part of the heap: one
// round trip, all lanes of the search wave.  Returns whether every such ancestor fits the cache.
__device__ __forceinline__ bool ancestor_cache_fill(const HeapRef& H, SearchLds& W, int lane, int n, int cnt)
{
    int nlev = 0, total = 0;
    int my_idx[2] = {-1, -1};
    bool complete = true;
    for (int j = 1; j <= SMPLX_AC_LEVELS; ++j) {
        int lo = (n + 1) >> j, hi = (n + cnt) >> j;
        if (hi > n) hi = n;
        if (hi < H.lh || cnt == 0) break;
        if (lo < H.lh) lo = H.lh;
        const int len = hi - lo + 1;
        if (total + len > SMPLX_AC_SLOTS || j == SMPLX_AC_LEVELS) { complete = false; break; }
        if (lane == 0) { W.ac_lo[j] = lo; W.ac_hi[j] = hi; W.ac_base[j] = total; }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int e = lane + 64 * r - total;
            if (e >= 0 && e < len) my_idx[r] = lo + e;
        }
        total += len;
        nlev = j;
    }
    if (lane == 0) W.ac_nlev = nlev;
#pragma unroll
    for (int r = 0; r < 2; ++r)
        if (my_idx[r] >= 0) W.ac_val[lane + 64 * r] = H.hbm[my_idx[r]];
    return complete;
}

// Parity-test kernel (test_hooks.h): the heap primitives of k_search driven by an op sequence in the language of
// oracle/heap_ref_driver.cpp -- 0 push(priority), 1 pop, 2 / 5 decrease / increase(element << 20 | priority), 3 erase(element),
// 4 re-prioritise everything and make() -- so that they can be compared with the reference's own intrusive_heap
// (tests/golden/heap_ref.json).  Element e is state e; the first `lh` heap entries live in LDS, the rest in HBM.  One wave:
// push / decrease run the wave-parallel sift-up, pop is the search's heap_pop_wave, increase / erase run the wave-parallel
// sift-down, make() the level-parallel form -- the code paths of the search.
extern "C" __global__ void __launch_bounds__(64)
k_heap_ops(const int* __restrict__ ops, int nops, int lh, unsigned long long* __restrict__ heap_hbm, SmplxSState* __restrict__ st,
           int* __restrict__ top_after)
{
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ SearchLds W;
    HeapRef H;
    H.lds = (LDS_AS hent_t*)smem;
    H.hbm = as_global(heap_hbm);
    H.st = as_global(st);
    H.lh = lh;
    const int lane = threadIdx.x;
    if (lane == 0) W.ac_nlev = 0;
    __syncthreads();
    int nelem = 0, size = 0;
    for (int i = 0; i < nops; ++i) {
        const int code = ops[2 * i], key = ops[2 * i + 1];
        if (code == 0) {
            if (lane == 0) { st[nelem].f = (unsigned int)key; st[nelem].heap_index = 0; }
            ++size;
            heap_sift_up_wave(H, W, lane, size, hent_make((unsigned int)key, nelem), false);
            ++nelem;
        } else if (code == 1) {
            if (size > 0) {
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                const hent_t top = hget(H, 1), last = hget(H, size);
                heap_pop_wave(H, lane, hent_id(top), size, last);
            }
        } else if (code == 2 || code == 5) {
            const int e = key >> 20, p = key & 0xFFFFF;
            const int hi = e < nelem ? st[e].heap_index : 0;
            if (hi != 0) {
                if (lane == 0) st[e].f = (unsigned int)p;
                if (code == 2) heap_sift_up_wave(H, W, lane, hi, hent_make((unsigned int)p, e), false);
                else heap_sift_down_wave(H, lane, hi, size, hent_make((unsigned int)p, e));
            }
        } else if (code == 3) {
            const int pos = key < nelem ? st[key].heap_index : 0;
            if (pos != 0) {                                      // intrusive_heap.hpp:197-206
                const hent_t last = hget(H, size);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                if (lane == 0) { hset(H, pos, last); st[key].heap_index = 0; }
                --size;
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                if (pos <= size) heap_sift_down_wave(H, lane, pos, size, last);
            }
        } else if (code == 4) {
            for (int k = 1 + lane; k <= size; k += 64) {
                const int e = hent_id(hget(H, k));
                const unsigned int p = (st[e].f * 7919u + 13u) % 1000u;
                st[e].f = p;
                hput(H, k, hent_make(p, e));
            }
            __syncthreads();
            heap_make_block(H, size, false);
        }
        __syncthreads();      // (one wave: orders what the lanes stored with what the next op reads)
        if (lane == 0) top_after[i] = size > 0 ? hent_id(hget(H, 1)) : -1;
    }
}
