// smpl_amd/csrc/ara_search.h -- the host-driven ARA*, the caller of GetSuccs (smpl/src/search/arastar.cpp).
// Sequential and bit-faithful: OPEN is the intrusive binary heap of smpl/include/smpl/detail/intrusive_heap.hpp
// (strict '<' sift rules), keys are g + (unsigned)(eps*h).  The only addition is the frontier hint before a cache
// miss.  Search is a resumable state machine: resume() runs until the search finishes or a frontier batch is in flight.
#pragma once

#include <algorithm>
#include <chrono>
#include <cstring>
#include <limits>
#include <vector>

#include "space.h"
#include "step.h"

namespace {

const unsigned int kInfiniteCost = 1000000000u;   // SBPL INFINITECOST

struct SearchState {
    unsigned int g, h, f, eg;
    unsigned short iteration_closed, call_number;
    int bp;
    int heap_index;
    bool incons;
    bool made;
};

struct Search {
    smplx_space* sp;
    std::vector<SearchState> st;
    std::vector<int> heap;      // heap[0] unused
    std::vector<int> incons;
    double curr_eps = 1.0, initial_eps = 1.0, final_eps = 1.0, delta_eps = 1.0;
    bool improve = true, bounded = false;
    int max_init = 0, max_rep = 0;
    int iteration = 1, call_number = 0;
    double satisfied_eps = std::numeric_limits<double>::infinity();
    int expand_count = 0, expand_count_init = 0;
    int start_id = -1, goal_id = 0;
    int error = SMPLX_OK;
    bool wall = false, allow_partial = false;      // smplx_time_params: wall-clock budget, partial solutions
    double max_sec_init = 0.0, max_sec_rep = 0.0;
    std::chrono::steady_clock::time_point t_call;  // when the call began (the wall-clock budget's clock)

    bool less(int a, int b) const { return st[a].f < st[b].f; }
    bool heap_empty() const { return heap.size() == 1; }
    void heap_clear() { for (size_t i = 1; i < heap.size(); ++i) st[heap[i]].heap_index = 0; heap.resize(1); }
    void percolate_down(size_t pivot)   // intrusive_heap.hpp:346-377
    {
        if (pivot >= heap.size()) return;
        size_t left = pivot << 1, right = (pivot << 1) + 1;
        const int tmp = heap[pivot];
        while (left < heap.size()) {
            size_t c = right;
            if (right >= heap.size() || less(heap[left], heap[right])) c = left;
            if (less(heap[c], tmp)) {
                heap[pivot] = heap[c];
                st[heap[pivot]].heap_index = (int)pivot;
                pivot = c;
            } else break;
            left = pivot << 1; right = (pivot << 1) + 1;
        }
        heap[pivot] = tmp;
        st[tmp].heap_index = (int)pivot;
    }
    void percolate_up(size_t pivot)     // intrusive_heap.hpp:379-395
    {
        const int tmp = heap[pivot];
        while (pivot != 1) {
            const size_t p = pivot >> 1;
            if (less(heap[p], tmp)) break;
            heap[pivot] = heap[p];
            st[heap[pivot]].heap_index = (int)pivot;
            pivot = p;
        }
        heap[pivot] = tmp;
        st[tmp].heap_index = (int)pivot;
    }
    void push(int e) { st[e].heap_index = (int)heap.size(); heap.push_back(e); percolate_up(heap.size() - 1); }
    void pop()
    {
        st[heap[1]].heap_index = 0;
        heap[1] = heap.back();
        heap.pop_back();
        percolate_down(1);
    }
    void make() { for (size_t i = (heap.size() - 1) >> 1; i >= 1; --i) percolate_down(i); }

    SearchState& get(int id)
    {
        if ((int)st.size() <= id) {
            SearchState z;
            std::memset(&z, 0, sizeof(z));
            st.resize(id + 1, z);
        }
        if (!st[id].made) { st[id].made = true; st[id].call_number = 0; st[id].heap_index = 0; }
        return st[id];
    }
    void reinit(int id)   // arastar.cpp:613-627
    {
        SearchState& s = get(id);
        if (s.call_number != (unsigned short)call_number) {
            int32_t h = 0;
            smplx_get_goal_heuristic(sp, id, &h);
            s.g = kInfiniteCost;
            s.h = (unsigned int)h;
            s.f = kInfiniteCost;
            s.eg = kInfiniteCost;
            s.iteration_closed = 0;
            s.call_number = (unsigned short)call_number;
            s.bp = -1;
            s.incons = false;
        }
    }
    unsigned int key(const SearchState& s) const { return s.g + (unsigned int)(long long)(curr_eps * s.h); }   // :579-582
    void reorder_open()
    {
        for (size_t i = 1; i < heap.size(); ++i) st[heap[i]].f = key(st[heap[i]]);
        make();
    }
    bool timed_out(int elapsed) const   // arastar.cpp:454-484
    {
        if (!bounded) return false;
        const bool init = satisfied_eps == std::numeric_limits<double>::infinity();
        if (wall) return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_call).count() >= (init ? max_sec_init : max_sec_rep);
        return elapsed >= (init ? max_init : max_rep);
    }
    void expand(int sid)   // arastar.cpp:531-568
    {
        const int32_t *succs, *costs;
        int n = 0;
        error = get_succs(sp, sid, &succs, &costs, &n);   // served from the cache: improve_path checked ready(sid)
        if (error) return;
        // succs/costs point into the committed arrays, which only get_succs grows: nothing below calls it
        const int32_t* ss = succs;
        const int32_t* cc = costs;
        const unsigned int eg = st[sid].eg;
        for (int i = 0; i < n; ++i)
            if ((size_t)ss[i] < st.size()) __builtin_prefetch(&st[ss[i]]);   // the successors' search states, all misses at once
        for (int i = 0; i < n; ++i) {
            const int nid = ss[i];
            reinit(nid);
            SearchState& t = st[nid];
            const int new_cost = (int)(eg + (unsigned int)cc[i]);
            if ((unsigned int)new_cost < t.g) {
                t.g = (unsigned int)new_cost;
                t.bp = sid;
                if (t.iteration_closed != (unsigned short)iteration) {
                    t.f = key(t);
                    if (t.heap_index != 0) percolate_up(t.heap_index);
                    else push(nid);
                } else if (!t.incons) {
                    incons.push_back(nid);
                }
            }
        }
    }
    // states whose successors are already on the host (cached or committed); the goal never expands
    bool ready(int sid) const { return sid == 0 || sp->lat.done_off[sid] >= 0 || sp->lat.cache_off[sid] >= 0; }

    enum { R_DONE = 0, R_YIELD = 100 };
    int hint_scan = 1024;  // entries of OPEN's array examined for the hint of a miss (SMPLX_HINT_SCAN)
    int pause_after = 0;   // > 0: hand control back after that many expansions without a miss (miss_id = -1): keeps the
                           // rounds of the pipelined multi-query driver even; the search resumes at exactly this point
    int improve_path(int& elapsed)   // arastar.cpp:486-527; returns R_YIELD when a frontier batch was issued
    {
        int since_entry = 0;
        while (!heap_empty()) {
            const int m = heap[1];
            if (st[m].f >= st[goal_id].f || m == goal_id) return 0;
            if (timed_out(elapsed)) return 4;
            if (pause_after > 0 && since_entry >= pause_after) { miss_id = -1; return R_YIELD; }
            ++since_entry;
            if (!ready(m)) {
                // cache miss: the state and the top of OPEN go to the GPU as one frontier batch; the search
                // resumes from exactly this point when the batch has landed (nothing has been popped yet)
                // the hint: the states near the top of OPEN that have not been evaluated yet.  Only the first `hint_scan`
                // entries of the heap array are looked at (the array is only roughly sorted, and what sits deep in it is not
                // expanded soon): scanning all of a 30 000-entry OPEN on every miss cost the single-query search ~10 us per miss
                const int cap = sp->params.batch_states > 0 ? sp->params.batch_states : 4096;
                sp->spec.hint.clear();
                const size_t scan_end = std::min(heap.size(), (size_t)2 + (size_t)hint_scan);
                for (size_t i = 2; i < scan_end && (int)sp->spec.hint.size() < cap - 1; ++i) {
                    const int hid = heap[i];
                    if (hid > 0 && sp->lat.cache_off[hid] == -1 && sp->lat.done_off[hid] < 0) sp->spec.hint.push_back(hid);
                }
                ++sp->cache_misses;
                miss_id = m;
                if (!defer_issue) {
                    error = issue_batch(sp, m);
                    if (error) return 99;
                }
                return R_YIELD;
            }
            pop();
            st[m].iteration_closed = (unsigned short)iteration;
            st[m].eg = st[m].g;
            sp->expansion_log.push_back(m);
            expand(m);
            if (error) return 99;
            ++elapsed;
        }
        return 5;
    }

    // arastar.cpp:107-215 as a resumable state machine: resume() runs until the search finishes (R_DONE) or a frontier
    // batch is in flight (R_YIELD).  Phase 0 starts from scratch; continue_call() re-enters a finished search at phase 1
    // for a later call (smplx_replan), which keeps OPEN, INCONS, the search states, iteration and epsilons
    int phase = 0, num = 0, err = 0, solved = 0, cost = 0;
    std::vector<int> solution;
    void continue_call()
    {
        phase = 1; num = 0; err = 0; solved = 0; cost = 0;
        solution.clear();
        error = SMPLX_OK; miss_id = -1;
        defer_issue = false; pause_after = 0;       // (set again by the multi-query drivers)
    }
    int resume()
    {
        if (phase == 0) {
            heap.assign(1, 0);
            incons.clear();
            ++call_number;
            reinit(start_id);
            reinit(goal_id);
            st[start_id].g = 0;
            st[start_id].f = key(st[start_id]);
            push(start_id);
            iteration = 1;
            curr_eps = initial_eps;
            satisfied_eps = std::numeric_limits<double>::infinity();
            // goal id "changed" on a fresh search: recompute h of existing states and reorder (:155-162)
            for (size_t i = 0; i < st.size(); ++i) {
                if (st[i].made) { int32_t h = 0; smplx_get_goal_heuristic(sp, (int)i, &h); st[i].h = (unsigned int)h; }
            }
            reorder_open();
            num = 0; err = 0;
            phase = 1;
        }
        while (true) {
            if (phase == 1) {
                if (!(satisfied_eps > final_eps)) break;
                if (curr_eps == satisfied_eps) {
                    if (!improve) break;
                    ++iteration;
                    curr_eps -= delta_eps;
                    curr_eps = std::max(curr_eps, final_eps);
                    for (int s : incons) { st[s].incons = false; push(s); }
                    reorder_open();
                    incons.clear();
                }
                phase = 2;
                num_before = num;
            }
            err = improve_path(num);
            if (err == R_YIELD) return R_YIELD;
            if (curr_eps == initial_eps) expand_count_init += num;
            phase = 1;
            if (err) break;
            satisfied_eps = curr_eps;
        }
        expand_count += num;
        phase = 3;
        // arastar.cpp:199-214: the goal's chain once there is a solution, else with partial solutions the chain of OPEN's minimum
        int from = -1;
        if (satisfied_eps != std::numeric_limits<double>::infinity()) from = goal_id;
        else if (allow_partial && !heap_empty()) from = heap[1];
        if (from < 0) { solved = 0; return R_DONE; }
        for (int s = from; s >= 0; s = st[s].bp) solution.push_back(s);
        std::reverse(solution.begin(), solution.end());
        cost = (int)st[from].g;
        solved = 1;
        return R_DONE;
    }
    int num_before = 0;
    int miss_id = -1;
    bool defer_issue = false;   // cross-query batching: the caller gathers the misses of many queries into one launch
};

// the parameters a call may change (a resumed call too: the reference's setters between calls)
void set_call_params(Search& S, const smplx_time_params* p, std::chrono::steady_clock::time_point t_call)
{
    S.final_eps = std::max(p->final_eps, 1.0);   // ARAStar::setTargetEpsilon (arastar.h:112-114)
    S.delta_eps = p->delta_eps;
    S.improve = p->improve != 0;
    S.bounded = p->bounded != 0;
    S.max_init = p->max_expansions_init;
    S.max_rep = p->max_expansions;
    S.wall = p->type == SMPLX_TIME_WALL;
    S.max_sec_init = p->max_seconds_init;
    S.max_sec_rep = p->max_seconds;
    S.allow_partial = p->allow_partial != 0;
    S.t_call = t_call;
}

void fill_search(Search& S, smplx_space* s, const smplx_time_params* p, std::chrono::steady_clock::time_point t_call)
{
    S.sp = s;
    S.initial_eps = p->initial_eps;
    set_call_params(S, p, t_call);
    S.start_id = s->lat.start_id;
    S.goal_id = 0;
}

}  // namespace
