// smpl_amd/csrc/path_multi.h -- host side of smplx_post_process_paths: PlannerInterface::postProcessPath
// (planner_interface.cpp:2651-2697) for a batch of paths in a bounded number of launches (kernels: path_kernels.h).
// A call is at most three stages, each ONE launch and ONE wait whatever the batch holds:
//   interpolate  the host interpolates every edge of every path with the single call's arithmetic (PathTools over
//                smplx_cc_interpolate, path_tools.h), k_paths_valid checks all waypoints of all paths -- each path against
//                its own space -- and the host assembles the outputs as interpolate_path does
//   shortcut     the host sums the accumulated costs (PathTools::distance), k_shortcut runs the greedy loop of every
//                path to its end on the device and returns the indices of the points it keeps
//   interpolate  again, over the shortcut paths
// Sizes are exact, not bounded: the host knows every row count before it launches, so nothing can overflow on the
// device and no path is ever truncated (last_pass_bound below is checked by the tests, not relied on).
// The first part of this file is plain arithmetic over the caller's offsets and needs no HIP: tests/cpp/
// path_multi_host_driver.cpp compiles it alone (SMPLX_PATH_MULTI_ARITHMETIC_ONLY).
#pragma once

#include <climits>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace smplx_path_multi {

// the caller's offsets: nq + 1 entries in points, first[0] == 0, non-decreasing.  Returns false for anything else;
// *total = first[nq].  (An int32 offset cannot exceed INT_MAX; the products with nvars are taken in 64 bits.)
inline bool check_offsets(const int32_t* first, int nq, long long* total)
{
    if (!first || nq < 0 || first[0] != 0) return false;
    for (int k = 0; k < nq; ++k)
        if (first[k + 1] < first[k]) return false;
    if (total) *total = first[nq];
    return true;
}

// out_first from the per-path output sizes; false when a sum does not fit the int32 offsets (nothing is written then)
inline bool output_offsets(const long long* counts, int nq, int32_t* out_first)
{
    long long sum = 0;
    for (int k = 0; k < nq; ++k) {
        if (counts[k] < 0 || counts[k] > INT_MAX - sum) return false;
        sum += counts[k];
    }
    out_first[0] = 0;
    for (int k = 0; k < nq; ++k) out_first[k + 1] = out_first[k] + (int32_t)counts[k];
    return true;
}

// The last pass against the first.  rows = the waypoints the first pass has to check for the path: the sum of
// edge_waypoint_count over the edges of the input path of P points.  A shortcut edge's motion is at most the sum of the
// motions it replaces, so its waypoint count less one is at most the sum of theirs; an edge that the first pass
// interpolated has become sub-edges of two waypoints each (three where the division rounds up), an edge it found in
// collision stayed whole.  Either way the points the last pass writes are at most 2 * rows + P.
// (Not the first pass's OUTPUT size: an edge in collision leaves one point there, and a free shortcut across it is
// interpolated in full.  A batch of 300 random zig-zags showed 404 points behind a first pass of 149.)
inline long long last_pass_bound(long long rows, long long P) { return 2 * rows + P; }

// the block table of k_paths_valid: (path, first row, rows <= block) per block, a path's rows in blocks of their own
inline void append_blocks(std::vector<int32_t>& blocks, int path, long long row0, long long rows, int block)
{
    for (long long r = 0; r < rows; r += block) {
        blocks.push_back(path);
        blocks.push_back((int32_t)(row0 + r));
        blocks.push_back((int32_t)(rows - r < block ? rows - r : block));
    }
}

}  // namespace smplx_path_multi

#ifndef SMPLX_PATH_MULTI_ARITHMETIC_ONLY

#include <cstring>
#include <string>

#include "kernels.h"
#include "path_tools.h"
#include "space.h"

namespace {

// what two spaces of one call must share: the grid, the model image and the kernel build (multi_query.h
// same_scene_and_robot without the primitives and the heuristic kind, which no kernel of this call reads)
bool same_grid_and_robot(const smplx_space* a, const smplx_space* b)
{
    return a->grid == b->grid && a->device == b->device && a->N == b->N && a->blob_bytes == b->blob_bytes &&
           std::memcmp(a->hs.model_blob, b->hs.model_blob, a->blob_bytes) == 0 && a->ks.specialized == b->ks.specialized;
}

struct PathBatch {
    smplx_space* lead;
    smplx_space* const* spaces;
    int nq, N;
    std::vector<std::vector<double>> paths;      // the paths as they stand between the stages
    int64_t launches = 0, waits = 0, configs = 0;
    std::vector<const SmplxSpaceDev*> tab;       // per path: its space's device image
    bool tab_uploaded = false;

    // the table of the paths' space images (the stab of k_table_insert is the precedent), uploaded once a call, in front
    // of its first launch: the stage that launches also waits, so the copy has read `tab` before the call returns
    int upload_stab()
    {
        if (tab_uploaded) return SMPLX_OK;
        tab.resize(nq);
        for (int k = 0; k < nq; ++k) tab[k] = spaces[k]->d_space;
        if (int e = reserve(lead->pm.b_stab, (size_t)nq)) return e;
        HIP_TRY(hipMemcpyAsync(lead->pm.b_stab.p, tab.data(), sizeof(void*) * nq, hipMemcpyHostToDevice, lead->stream));
        tab_uploaded = true;
        return SMPLX_OK;
    }

    // post_processing.cpp:464-523 over CollisionSpace::interpolatePath for every path: interpolate_path of path_tools.h
    // with the validity of all rows asked in one launch
    int interpolate_all(bool fork_limits_test)
    {
        PathMultiHost& W = lead->pm;
        std::vector<double> q;                        // waypoints of every edge of every path that is interpolated
        std::vector<std::vector<int>> first(nq);      // per path: row offsets of its edges, empty when it stays as it is
        std::vector<int32_t> blocks;
        for (int k = 0; k < nq; ++k) {
            PathTools T(spaces[k]);
            const std::vector<double>& path = paths[k];
            const int P = (int)(path.size() / N);
            if (P == 0) continue;
            bool done = true;
            for (int i = 0; i + 1 < P && done; ++i) {
                const double* a = path.data() + (size_t)i * N;
                const bool wa = T.within_limits(a), wb = T.within_limits(a + N);
                // [FORK] :592-597 reports "Joint limits violated" when either end IS within its limits
                if (fork_limits_test ? (wa || wb) : (!wa || !wb)) done = false;
            }
            if (!done) continue;                      // the reference's failure: the path stays as it was
            const size_t row0 = q.size() / N;
            std::vector<int>& f = first[k];
            f.assign(1, (int)row0);
            for (int i = 0; i + 1 < P; ++i) {
                const double* a = path.data() + (size_t)i * N;
                const int Wn = T.waypoint_count(a, a + N);
                if (q.size() / N + (size_t)Wn > (size_t)INT_MAX) return set_error(SMPLX_E_LIMIT, "the waypoints of the batch do not fit 32-bit row offsets");
                T.append_waypoints(a, a + N, Wn, q);
                f.push_back(f.back() + Wn);
            }
            smplx_path_multi::append_blocks(blocks, k, (long long)row0, (long long)(q.size() / N - row0), SMPLX_BLOCK);
        }
        const size_t rows = q.size() / N;
        std::vector<uint8_t> valid(rows, 0);
        if (rows > 0) {
            int e;
            if ((e = upload_stab())) return e;
            if ((e = reserve(W.b_rows, q.size()))) return e;
            if ((e = reserve(W.b_valid, rows))) return e;
            if ((e = reserve(W.b_ints, blocks.size()))) return e;
            HIP_TRY(hipMemcpyAsync(W.b_rows.p, q.data(), sizeof(double) * q.size(), hipMemcpyHostToDevice, lead->stream));
            HIP_TRY(hipMemcpyAsync(W.b_ints.p, blocks.data(), sizeof(int32_t) * blocks.size(), hipMemcpyHostToDevice, lead->stream));
            KLAUNCH(lead, K_PATHS_VALID, k_paths_valid, dim3((unsigned)(blocks.size() / 3)), dim3(SMPLX_BLOCK), lead->lds_bytes_valid,
                    lead->stream, W.b_stab.p, W.b_ints.p, W.b_rows.p, W.b_valid.p);
            HIP_TRY(hipGetLastError());
            ++launches;
            HIP_TRY(hipMemcpyAsync(valid.data(), W.b_valid.p, rows, hipMemcpyDeviceToHost, lead->stream));
            HIP_TRY(hipStreamSynchronize(lead->stream));
            ++waits;
            configs += (int64_t)rows;
        }
        for (int k = 0; k < nq; ++k) {
            const std::vector<int>& f = first[k];
            if (f.empty()) continue;
            std::vector<double>& path = paths[k];
            const int P = (int)(path.size() / N);
            std::vector<double> out(path.begin(), path.begin() + N);
            for (int i = 0; i + 1 < P; ++i) {
                bool collision = false;
                for (int w = f[i]; w < f[i + 1]; ++w) collision = collision || valid[w] == 0;
                if (collision) {
                    out.insert(out.end(), path.begin() + (size_t)(i + 1) * N, path.begin() + (size_t)(i + 2) * N);
                } else if (f[i + 1] > f[i]) {
                    out.insert(out.end(), q.begin() + (size_t)(f[i] + 1) * N, q.begin() + (size_t)f[i + 1] * N);
                }
            }
            path.swap(out);
        }
        return SMPLX_OK;
    }

    // shortcut_path of path_tools.h for every path: the accumulated costs here, the loop in k_shortcut
    int shortcut_all()
    {
        PathMultiHost& W = lead->pm;
        std::vector<double> pts, accum;
        std::vector<int32_t> first(nq + 1, 0);
        for (int k = 0; k < nq; ++k) {
            const std::vector<double>& p = paths[k];
            const int P = (int)(p.size() / N);
            if (pts.size() / N + (size_t)P > (size_t)INT_MAX) return set_error(SMPLX_E_LIMIT, "the points of the batch do not fit 32-bit offsets");
            PathTools T(spaces[k]);
            accum.push_back(0.0);
            if (P == 0) accum.pop_back();
            for (int i = 1; i < P; ++i) accum.push_back(accum.back() + T.distance(p.data() + (size_t)(i - 1) * N, p.data() + (size_t)i * N));
            pts.insert(pts.end(), p.begin(), p.end());
            first[k + 1] = first[k] + P;
        }
        const size_t total = (size_t)first[nq];
        if (total == 0) return SMPLX_OK;
        // ints: first[nq + 1] | keep[total] | nkeep[nq] | err[nq]
        const size_t o_keep = (size_t)nq + 1, o_nkeep = o_keep + total, o_err = o_nkeep + nq, n_ints = o_err + nq;
        int e;
        if ((e = upload_stab())) return e;
        if ((e = reserve(W.b_rows, pts.size() + accum.size()))) return e;
        if ((e = reserve(W.b_ints, n_ints))) return e;
        if ((e = reserve(W.b_checked, (size_t)nq))) return e;
        double* d_pts = W.b_rows.p;
        double* d_accum = W.b_rows.p + pts.size();
        HIP_TRY(hipMemcpyAsync(d_pts, pts.data(), sizeof(double) * pts.size(), hipMemcpyHostToDevice, lead->stream));
        HIP_TRY(hipMemcpyAsync(d_accum, accum.data(), sizeof(double) * accum.size(), hipMemcpyHostToDevice, lead->stream));
        HIP_TRY(hipMemcpyAsync(W.b_ints.p, first.data(), sizeof(int32_t) * first.size(), hipMemcpyHostToDevice, lead->stream));
        KLAUNCH(lead, K_SHORTCUT, k_shortcut, dim3((unsigned)nq), dim3(SMPLX_BLOCK), lead->lds_bytes_valid, lead->stream, W.b_stab.p, d_pts,
                W.b_ints.p, d_accum, W.b_ints.p + o_keep, W.b_ints.p + o_nkeep, W.b_ints.p + o_err, W.b_checked.p);
        HIP_TRY(hipGetLastError());
        ++launches;
        std::vector<int32_t> back(n_ints - o_keep);
        std::vector<long long> checked(nq);
        HIP_TRY(hipMemcpyAsync(back.data(), W.b_ints.p + o_keep, sizeof(int32_t) * back.size(), hipMemcpyDeviceToHost, lead->stream));
        HIP_TRY(hipMemcpyAsync(checked.data(), W.b_checked.p, sizeof(long long) * nq, hipMemcpyDeviceToHost, lead->stream));
        HIP_TRY(hipStreamSynchronize(lead->stream));
        ++waits;
        const int32_t* keep = back.data();
        const int32_t* nkeep = back.data() + total;
        const int32_t* err = nkeep + nq;
        for (int k = 0; k < nq; ++k) {
            const int P = first[k + 1] - first[k];
            if (err[k] != 0 || nkeep[k] < 0 || nkeep[k] > P)
                return set_error(SMPLX_E_HIP, "k_shortcut: path " + std::to_string(k) +
                                                  (err[k] == 1 ? " exceeded the trip bound 2P + 2" : " overflowed its keep list"));
            configs += (int64_t)checked[k];
            std::vector<double> out;
            out.reserve((size_t)nkeep[k] * N);
            int last = -1;
            for (int i = 0; i < nkeep[k]; ++i) {
                const int idx = keep[first[k] + i];
                if (idx <= last || idx >= P) return set_error(SMPLX_E_HIP, "k_shortcut: path " + std::to_string(k) + " returned indices out of order");
                last = idx;
                out.insert(out.end(), paths[k].begin() + (size_t)idx * N, paths[k].begin() + (size_t)(idx + 1) * N);
            }
            paths[k].swap(out);
        }
        return SMPLX_OK;
    }
};

int post_process_paths(smplx_space* const* spaces, int nq, const double* pts, const int32_t* first, int flags, double* out, int cap,
                       int32_t* out_first, int64_t* stats)
{
    smplx_space* lead = spaces[0];
    const int N = lead->N;
    HIP_TRY(hipSetDevice(lead->device));
    PathBatch B{lead, spaces, nq, N};
    B.paths.resize(nq);
    for (int k = 0; k < nq; ++k) B.paths[k].assign(pts + (size_t)first[k] * N, pts + (size_t)first[k + 1] * N);
    const bool fork_test = !(flags & SMPLX_PP_UPSTREAM_LIMITS);
    // PlannerInterface::postProcessPath (planner_interface.cpp:2651-2697)
    if (flags & SMPLX_PP_SHORTCUT) {
        if (int e = B.interpolate_all(fork_test)) return e;   // failure leaves a path as it was
        if (int e = B.shortcut_all()) return e;
    }
    if (flags & SMPLX_PP_INTERPOLATE) {
        if (int e = B.interpolate_all(fork_test)) return e;
    }
    std::vector<long long> counts(nq);
    for (int k = 0; k < nq; ++k) counts[k] = (long long)(B.paths[k].size() / N);
    std::vector<int32_t> of(nq + 1);
    if (!smplx_path_multi::output_offsets(counts.data(), nq, of.data())) return set_error(SMPLX_E_LIMIT, "the output does not fit 32-bit offsets");
    std::memcpy(out_first, of.data(), sizeof(int32_t) * (nq + 1));
    if (stats) { stats[0] = B.launches; stats[1] = B.waits; stats[2] = B.configs; stats[3] = nq; }
    if (out) {
        if (of[nq] > cap) return set_error(SMPLX_E_LIMIT, "output paths do not fit");
        for (int k = 0; k < nq; ++k)
            if (!B.paths[k].empty()) std::memcpy(out + (size_t)of[k] * N, B.paths[k].data(), sizeof(double) * B.paths[k].size());
    }
    return SMPLX_OK;
}

}  // namespace

#endif  // SMPLX_PATH_MULTI_ARITHMETIC_ONLY
