// smpl_amd/csrc/lattice.h -- the host's ManipLattice state table: states in commit order (manip_lattice.cpp:1302-1354) and
// everything indexed by state id -- coordinates, joint values, heuristic, the coordinate -> id hash, the speculative
// successor cache, the committed successor lists.  Lattice is the only code that changes the length of a per-id array:
// clear() starts a query and reserves id 0, append() commits one state, extend() makes room for the states the
// device-resident search created.  A per-id array added later is added to the member list and to grow(), nowhere else.
#pragma once

#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "det_math.h"
#include "device_types.h"

namespace {

// host mirror of ManipLattice::stateToCoord (manip_lattice.cpp:1263-1289) on det_math
void state_to_coord(const SmplxModelDev& m, const double* q, int32_t* c)
{
    for (int v = 0; v < m.nvars; ++v) {
        const double delta = m.coord_delta[v];
        if (m.var_type[v] == SMPLX_JT_CONTINUOUS) {
            const double pos = smplx_normalize_angle_positive(q[v]);
            int k = (int)((pos + delta * 0.5) / delta);
            if (k == m.coord_vals[v]) k = 0;
            c[v] = k;
        } else {
            c[v] = (int)(((q[v] - m.var_min[v]) / delta) + 0.5);
        }
    }
}

// coord -> id table: open addressing over the commit-ordered coordinate array.  State ids depend
// only on insertion order (manip_lattice.cpp:1302-1354), never on the hash function.
struct CoordTable {
    int N = 0;
    std::vector<int32_t> slots;   // id + 1, 0 = empty
    size_t mask = 0, used = 0;
    void init(int n)
    {
        N = n;
        slots.assign(1 << 16, 0);
        mask = slots.size() - 1;
        used = 0;
    }
    static uint64_t hash(const int32_t* c, int n)
    {
        uint64_t h = 0x9E3779B97F4A7C15ull;
        for (int i = 0; i < n; ++i) {
            h ^= (uint64_t)(uint32_t)c[i] + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
            h *= 0xFF51AFD7ED558CCDull;
            h ^= h >> 33;
        }
        return h;
    }
    int find(const int32_t* c, const std::vector<int32_t>& coords) const { return find_hashed(c, hash(c, N), coords); }
    // the two dependent cache misses of a lookup (slot, then the coordinate row it names), started ahead of time
    void prefetch_slot(uint64_t h) const { __builtin_prefetch(&slots[h & mask]); }
    void prefetch_row(uint64_t h, const std::vector<int32_t>& coords) const
    {
        const int32_t s = slots[h & mask];
        if (s) __builtin_prefetch(&coords[(size_t)(s - 1) * N]);
    }
    int find_hashed(const int32_t* c, uint64_t h, const std::vector<int32_t>& coords) const
    {
        size_t i = h & mask;
        while (true) {
            const int32_t s = slots[i];
            if (s == 0) return -1;
            if (std::memcmp(&coords[(size_t)(s - 1) * N], c, sizeof(int32_t) * N) == 0) return s - 1;
            i = (i + 1) & mask;
        }
    }
    void insert(int id, const std::vector<int32_t>& coords)
    {
        if ((used + 1) * 2 > slots.size()) {
            std::vector<int32_t> old;
            old.swap(slots);
            slots.assign(old.size() * 2, 0);
            mask = slots.size() - 1;
            for (int32_t s : old) if (s) place(s - 1, coords);
        }
        place(id, coords);
        ++used;
    }
    void place(int id, const std::vector<int32_t>& coords)
    {
        size_t i = hash(&coords[(size_t)id * N], N) & mask;
        while (slots[i]) i = (i + 1) & mask;
        slots[i] = id + 1;
    }
};

struct Lattice {
    int N = 0;                          // variables per state
    std::vector<int32_t> coords;
    std::vector<double> qs;
    std::vector<int32_t> h_of_id;
    CoordTable table;
    int start_id = -1;
    // speculative successor cache (per state id: evaluated but not yet committed successors)
    struct Rec { int32_t cost; int32_t h; int32_t goal; int32_t known; int32_t prim; };
    std::vector<int64_t> cache_off;     // per id: first record, -1 = not evaluated
    std::vector<int32_t> cache_cnt;
    std::vector<Rec> recs;
    std::vector<int32_t> rec_coord;
    std::vector<double> rec_q;
    // committed successor lists (served on re-expansion in later ARA* iterations)
    std::vector<int64_t> done_off;
    std::vector<int32_t> done_cnt;
    std::vector<int32_t> done_succ, done_cost, done_prim;
    std::vector<int32_t> eval_count;    // per id: evaluated (active) primitives, for committed_evals
    std::vector<uint32_t> g_est;        // per id: the g-value a plain GetSuccs caller's expansions imply (PlainSpeculation)
    // lazy successors (GetLazySuccs, manip_lattice.cpp:1012-1090).  lazy_row: the state's row of k_lazy_succs outputs in
    // the lz_* arrays (M entries a row), evaluated by its own call or as a rider of another's, -1 = not evaluated.
    // lazy_off / lazy_cnt: its committed list in lazy_succ (0 for a goal successor) / lazy_goal / lazy_prim.
    std::vector<int64_t> lazy_row, lazy_off;
    std::vector<int32_t> lazy_cnt;
    std::vector<unsigned char> lz_flags;
    std::vector<int32_t> lz_coord, lz_h, lz_known;
    std::vector<double> lz_q;
    std::vector<int32_t> lazy_succ, lazy_prim;
    std::vector<unsigned char> lazy_goal;
    // GetTrueCost (manip_lattice.cpp:1094-1167): (parent id << 32 | child id) -> what k_true_cost answered
    struct TrueCost { int32_t cost, prim, nmatch; };
    std::unordered_map<uint64_t, TrueCost> true_cost;

    int size() const { return (int)h_of_id.size(); }

    // a new query: no states but the goal, id 0 (manip_lattice.cpp:122), which has no coordinate and is never hashed
    void clear(int n)
    {
        N = n;
        recs.clear(); rec_coord.clear(); rec_q.clear();
        done_succ.clear(); done_cost.clear(); done_prim.clear();
        lz_flags.clear(); lz_coord.clear(); lz_h.clear(); lz_known.clear(); lz_q.clear();
        lazy_succ.clear(); lazy_prim.clear(); lazy_goal.clear();
        true_cost.clear();
        table.init(N);
        start_id = -1;
        grow(0);
        grow(1);
    }
    // getOrCreateState's create branch: the next id, in the caller's sequential order
    int append(const int32_t* coord, const double* q, int32_t h)
    {
        const int id = size();
        grow((size_t)id + 1);
        std::memcpy(&coords[(size_t)id * N], coord, sizeof(int32_t) * N);
        std::memcpy(&qs[(size_t)id * N], q, sizeof(double) * N);
        h_of_id[id] = h;
        table.insert(id, coords);
        return id;
    }
    // room for the states [size(), total) that the device search created: the caller copies their coordinates, joint
    // values and heuristics in and then has them hashed with index_from(first new id)
    void extend(int total) { grow((size_t)total); }
    void index_from(int first) { for (int id = first; id < size(); ++id) table.insert(id, coords); }

private:
    // every per-id array, to `total` states: a new state is neither evaluated nor committed nor reached
    void grow(size_t total)
    {
        coords.resize(total * N, 0);
        qs.resize(total * N, 0.0);
        h_of_id.resize(total, 0);
        cache_off.resize(total, -1);
        cache_cnt.resize(total, 0);
        done_off.resize(total, -1);
        done_cnt.resize(total, 0);
        eval_count.resize(total, 0);
        g_est.resize(total, 1000000000u);
        lazy_row.resize(total, -1);
        lazy_off.resize(total, -1);
        lazy_cnt.resize(total, 0);
    }
};

}  // namespace
