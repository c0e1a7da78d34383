// smpl_amd/csrc/expand_entry.h -- the expansion entry points of the C-ABI over step.h and device_table.h: a batch of
// parents on host or device arrays, with or without the K5 outputs (successor ids, the compact stream), the sizes a
// caller of the _device forms allocates by, the device table's synchronisation, the tallies, the per-kernel timing, and
// the test hooks of the step and of the table (test_hooks.h).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "device_table.h"
#include "step.h"
#include "test_hooks.h"

namespace {

// the dense outputs of a batch of B parents from the space's scratch to the caller's arrays (each optional), on the
// space's stream; the caller synchronises
int expand_results(smplx_space* s, size_t BM, uint8_t* flags, int32_t* coord, double* succ_q, int32_t* h)
{
    if (flags) HIP_TRY(hipMemcpyAsync(flags, s->b_flags.p, BM, hipMemcpyDeviceToHost, s->stream));
    if (coord) HIP_TRY(hipMemcpyAsync(coord, s->b_coord.p, sizeof(int32_t) * BM * s->N, hipMemcpyDeviceToHost, s->stream));
    if (succ_q) HIP_TRY(hipMemcpyAsync(succ_q, s->b_sq.p, sizeof(double) * BM * s->N, hipMemcpyDeviceToHost, s->stream));
    if (h) HIP_TRY(hipMemcpyAsync(h, s->b_h.p, sizeof(int32_t) * BM, hipMemcpyDeviceToHost, s->stream));
    return SMPLX_OK;
}

// smplx_expand_batch_k5_device, plus the states to insert at the head of the step's first kernel (device memory)
int expand_k5_device(smplx_space* s, const double* d_q, int B, uint8_t* d_flags, int32_t* d_coord, double* d_succ_q,
                     int32_t* d_h, int32_t* d_cost, int32_t* d_lookups, int32_t* d_succ_id, int32_t* d_rec_a, int cap_a,
                     void* d_rec_b, int cap_b, int32_t* d_block_tab, int32_t* d_totals, void* d_work,
                     uint64_t* d_counters, void* stream, const int32_t* d_items, int n_items)
{
    if (!s || !d_q || !d_flags || !d_coord || !d_succ_q || !d_h || !d_cost || !d_lookups || !d_work || B <= 0)
        return set_error(SMPLX_E_ARG, "bad argument");
    if (d_rec_a && (!d_rec_b || !d_block_tab || !d_totals || cap_a < SMPLX_CMP_SHARDS || cap_b < SMPLX_CMP_SHARDS))
        return set_error(SMPLX_E_ARG, "incomplete compact-stream arguments");
    cap_a = cap_a / SMPLX_CMP_SHARDS * SMPLX_CMP_SHARDS;
    cap_b = cap_b / SMPLX_CMP_SHARDS * SMPLX_CMP_SHARDS;
    if (!s->goal.set) return set_error(SMPLX_E_STATE, "set a goal first");
    if (s->step.fused_mode && d_rec_a) return set_error(SMPLX_E_STATE, "the compact stream needs the pipeline kernels (not fused mode)");
    SmplxCompactDev cmp;
    std::memset(&cmp, 0, sizeof(cmp));
    cmp.rec_a = d_rec_a; cmp.rec_b = (unsigned char*)d_rec_b; cmp.block_tab = d_block_tab; cmp.totals = d_totals;
    cmp.cap_a = cap_a; cmp.cap_b = cap_b; cmp.rec_b_bytes = smplx_rec_b_bytes(s->N);
    K5Out k5;
    k5.d_id = d_succ_id;
    k5.cmp = d_rec_a ? &cmp : nullptr;
    k5.items = d_items;
    k5.n_items = n_items;
    ExpandArgs a;
    a.q = d_q; a.B = B;
    a.flags = d_flags; a.coord = d_coord; a.sq = d_succ_q; a.h = d_h; a.cost = d_cost; a.lookups = d_lookups;
    a.work = d_work;
    a.counters = (unsigned long long*)d_counters;
    a.stream = (hipStream_t)stream;
    a.k5 = &k5;
    return launch_expand(s, a);
}

}  // namespace

extern "C" {

int smplx_expand_batch(smplx_space* s, const double* q, int B, uint8_t* flags, int32_t* coord, double* succ_q, int32_t* h,
                       int32_t* cost, int32_t* lookups)
{
    if (!s || !q || B < 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (!s->goal.set) return set_error(SMPLX_E_STATE, "set a goal first (the primitives are gated by goal distance)");
    if (B == 0) return SMPLX_OK;
    if (!sane_values(q, (size_t)B * s->N)) return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    if (int e = reserve_expand(s, B)) return e;
    const size_t BM = (size_t)B * s->M;
    HIP_TRY(hipMemsetAsync(s->b_coord.p, 0, sizeof(int32_t) * BM * s->N, s->stream));
    HIP_TRY(hipMemsetAsync(s->b_sq.p, 0, sizeof(double) * BM * s->N, s->stream));
    HIP_TRY(hipMemcpyAsync(s->batch.b_q.p, q, sizeof(double) * B * s->N, hipMemcpyHostToDevice, s->stream));
    if (int e = smplx_expand_batch_device(s, s->batch.b_q.p, B, s->b_flags.p, s->b_coord.p, s->b_sq.p, s->b_h.p, s->batch.b_cost.p,
                                          s->batch.b_lookups.p, s->batch.b_work.p, nullptr, s->stream)) return e;
    if (int e = expand_results(s, BM, flags, coord, succ_q, h)) return e;
    if (cost) HIP_TRY(hipMemcpyAsync(cost, s->batch.b_cost.p, sizeof(int32_t) * BM, hipMemcpyDeviceToHost, s->stream));
    if (lookups) HIP_TRY(hipMemcpyAsync(lookups, s->batch.b_lookups.p, sizeof(int32_t) * BM, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return SMPLX_OK;
}

size_t smplx_expand_work_bytes(const smplx_space* s, int B)
{
    if (!s || B <= 0) return 0;
    return expand_work_bytes(B, s->M, s->N);
}

int smplx_expand_batch_device(smplx_space* s, const double* d_q, int B, uint8_t* d_flags, int32_t* d_coord, double* d_succ_q,
                              int32_t* d_h, int32_t* d_cost, int32_t* d_lookups, void* d_work, uint64_t* d_counters, void* stream)
{
    if (!s || !d_q || !d_flags || !d_coord || !d_succ_q || !d_h || !d_cost || !d_lookups || !d_work || B <= 0)
        return set_error(SMPLX_E_ARG, "bad argument");
    if (!s->goal.set) return set_error(SMPLX_E_STATE, "set a goal first");
    // the K5 launch without its outputs
    return smplx_expand_batch_k5_device(s, d_q, B, d_flags, d_coord, d_succ_q, d_h, d_cost, d_lookups, nullptr, nullptr, 0, nullptr, 0,
                                        nullptr, nullptr, d_work, d_counters, stream);
}

int smplx_table_sync(smplx_space* s)
{
    if (!s) return set_error(SMPLX_E_ARG, "null argument");
    if (int e = table_ensure(s)) return e;
    if (int e = table_flush(s, s->stream)) return e;
    HIP_TRY(hipStreamSynchronize(s->stream));
    return SMPLX_OK;
}

size_t smplx_compact_rec_b_bytes(const smplx_space* s) { return s ? (size_t)smplx_rec_b_bytes(s->N) : 0; }
int smplx_compact_blocks(const smplx_space* s, int B) { return s && B > 0 ? blocks_for((long long)B * s->M, SMPLX_BLOCK) : 0; }
int smplx_compact_totals_len(void) { return SMPLX_CMP_TOTALS; }
int smplx_compact_capacity(const smplx_space* s, int B)
{
    if (!s || B <= 0) return 0;
    const int nblocks = blocks_for((long long)B * s->M, SMPLX_BLOCK);
    return SMPLX_CMP_SHARDS * ((nblocks + SMPLX_CMP_SHARDS - 1) / SMPLX_CMP_SHARDS) * SMPLX_BLOCK;   // no sub-region can overflow
}

int smplx_expand_batch_k5_device(smplx_space* s, const double* d_q, int B, uint8_t* d_flags, int32_t* d_coord, double* d_succ_q,
                                 int32_t* d_h, int32_t* d_cost, int32_t* d_lookups, int32_t* d_succ_id, int32_t* d_rec_a, int cap_a,
                                 void* d_rec_b, int cap_b, int32_t* d_block_tab, int32_t* d_totals, void* d_work,
                                 uint64_t* d_counters, void* stream)
{
    return expand_k5_device(s, d_q, B, d_flags, d_coord, d_succ_q, d_h, d_cost, d_lookups, d_succ_id, d_rec_a, cap_a, d_rec_b, cap_b,
                            d_block_tab, d_totals, d_work, d_counters, stream, nullptr, 0);
}

int smplx_expand_batch_k5(smplx_space* s, const double* q, int B, uint8_t* flags, int32_t* coord, double* succ_q, int32_t* h,
                          int32_t* succ_id, int32_t* rec_a, int cap_a, void* rec_b, int cap_b, int32_t* block_tab, int32_t totals[3])
{
    if (!s || !q || B <= 0 || !rec_a || !rec_b || !block_tab || !totals || cap_a <= 0 || cap_b <= 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (!s->goal.set) return set_error(SMPLX_E_STATE, "set a goal first");
    if (!sane_values(q, (size_t)B * s->N)) return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    if (int e = reserve_expand(s, B)) return e;
    const size_t BM = (size_t)B * s->M;
    const size_t rb = (size_t)smplx_rec_b_bytes(s->N);
    const int nblocks = blocks_for((long long)BM, SMPLX_BLOCK);
    int e;
    if ((e = reserve(s->b_way, BM))) return e;                                       // dense ids
    if ((e = reserve(s->dt.b_ins, 2 * (size_t)cap_a + 4 * (size_t)nblocks + SMPLX_CMP_TOTALS))) return e;   // A records | block table | totals
    if ((e = reserve(s->batch.b_out, rb * (size_t)cap_b))) return e;                       // B records
    if ((e = table_ensure(s))) return e;
    // the states committed since the last batch ride with the step's first kernel, behind the parents in the same
    // buffer, as they do in a search's own batches (issue_frontier)
    if ((e = table_grow_if_needed(s))) return e;
    std::vector<int32_t>& items = s->batch.ins_items;   // stays put until the synchronise below
    items.clear();
    table_take_pending(s, 0, items);
    const size_t parent_doubles = (size_t)B * s->N;
    if ((e = reserve(s->batch.b_q, parent_doubles + (items.size() + 1) / 2))) return e;
    int32_t* d_a = s->dt.b_ins.p;
    int32_t* d_bt = d_a + 2 * (size_t)cap_a;
    int32_t* d_tot = d_bt + 4 * (size_t)nblocks;
    HIP_TRY(hipMemcpyAsync(s->batch.b_q.p, q, sizeof(double) * parent_doubles, hipMemcpyHostToDevice, s->stream));
    if (!items.empty())
        HIP_TRY(hipMemcpyAsync(s->batch.b_q.p + parent_doubles, items.data(), sizeof(int32_t) * items.size(), hipMemcpyHostToDevice, s->stream));
    if ((e = expand_k5_device(s, s->batch.b_q.p, B, s->b_flags.p, s->b_coord.p, s->b_sq.p, s->b_h.p, s->batch.b_cost.p, s->batch.b_lookups.p,
                              s->b_way.p, d_a, cap_a, s->batch.b_out.p, cap_b, d_bt, d_tot, s->batch.b_work.p, nullptr, s->stream,
                              (const int32_t*)(s->batch.b_q.p + parent_doubles), (int)(items.size() / ((size_t)s->N + 2))))) return e;
    if ((e = expand_results(s, BM, flags, coord, succ_q, h))) return e;
    if (succ_id) HIP_TRY(hipMemcpyAsync(succ_id, s->b_way.p, sizeof(int32_t) * BM, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(rec_a, d_a, sizeof(int32_t) * 2 * (size_t)cap_a, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(rec_b, s->batch.b_out.p, rb * (size_t)cap_b, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(block_tab, d_bt, sizeof(int32_t) * 4 * (size_t)nblocks, hipMemcpyDeviceToHost, s->stream));
    int32_t raw[SMPLX_CMP_TOTALS];
    HIP_TRY(hipMemcpyAsync(raw, d_tot, sizeof(raw), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    totals[0] = totals[1] = 0;
    for (int k = 0; k < SMPLX_CMP_SHARDS; ++k) { totals[0] += raw[32 * k]; totals[1] += raw[32 * k + 1]; }
    totals[2] = raw[32 * SMPLX_CMP_SHARDS];
    return SMPLX_OK;
}

size_t smplx_counters_bytes(const smplx_space* s, int B)
{
    if (!s || B <= 0) return 0;
    return counter_words(B, s->M) * sizeof(unsigned long long);
}

int smplx_counters_read(const smplx_space* s, const uint64_t* d_counters, int B, uint64_t out[6])
{
    if (!s || !d_counters || !out || B <= 0) return set_error(SMPLX_E_ARG, "bad argument");
    const size_t cw = counter_words(B, s->M);
    std::vector<unsigned long long> part(cw);
    HIP_TRY(hipMemcpy(part.data(), d_counters, sizeof(unsigned long long) * cw, hipMemcpyDeviceToHost));
    for (int k = 0; k < SMPLX_TALLIES; ++k) out[k] = 0;
    for (size_t i = 0; i < cw; ++i) out[i % SMPLX_TALLIES] += part[i];
    return SMPLX_OK;
}

int smplx_profile_begin(smplx_space* s, int max_launches)
{
    if (!s || max_launches < 0) return set_error(SMPLX_E_ARG, "bad argument");
    s->step.prof_events.clear();
    s->step.prof_used = 0;
    for (int i = 0; i < 3 * max_launches; ++i) {
        DevEvent e;
        HIP_TRY(e.create());
        s->step.prof_events.push_back(std::move(e));
    }
    return SMPLX_OK;
}

int smplx_profile_end(smplx_space* s, double* prep_ms, double* expand_ms, int* launches)
{
    if (!s || !prep_ms || !expand_ms || !launches) return set_error(SMPLX_E_ARG, "null argument");
    double a = 0.0, b = 0.0;
    const int n = (int)(s->step.prof_used / 3);
    for (int i = 0; i < n; ++i) {
        float t = 0.f;
        HIP_TRY(hipEventSynchronize(s->step.prof_events[3 * i + 2]));
        HIP_TRY(hipEventElapsedTime(&t, s->step.prof_events[3 * i], s->step.prof_events[3 * i + 1]));
        a += t;
        HIP_TRY(hipEventElapsedTime(&t, s->step.prof_events[3 * i + 1], s->step.prof_events[3 * i + 2]));
        b += t;
    }
    *prep_ms = a; *expand_ms = b; *launches = n;
    s->step.prof_events.clear();
    s->step.prof_used = 0;
    return SMPLX_OK;
}

int smplx_test_set_work_list_items(smplx_space* s, int items)
{
    if (!s || items < 0) return set_error(SMPLX_E_ARG, "bad argument");
    s->step.work_list_items = items / 8 * 8;
    return SMPLX_OK;
}

int smplx_test_set_pipe_prep(smplx_space* s, int on)
{
    if (!s) return set_error(SMPLX_E_ARG, "null space");
    s->step.pipe_prep = on != 0;
    return SMPLX_OK;
}

int smplx_test_set_one_launch(smplx_space* s, int mode)
{
    if (!s || mode < -1 || mode > 1) return set_error(SMPLX_E_ARG, "bad argument");
    s->step.one_launch = mode;
    return SMPLX_OK;
}

long long smplx_test_one_launch_steps(const smplx_space* s) { return s ? (long long)s->step.one_launch_steps : -1; }

int smplx_test_step_counters_zero(smplx_space* s, void* stream)
{
    if (!s) return set_error(SMPLX_E_ARG, "null space");
    for (StepLaunch::WorkCounters& w : s->step.work_counters) {
        if (w.stream != (hipStream_t)stream) continue;
        std::vector<int32_t> h(SMPLX_WORK_COUNTER_BYTES / sizeof(int32_t));
        HIP_TRY(hipStreamSynchronize(w.stream));
        HIP_TRY(hipMemcpy(h.data(), w.p, SMPLX_WORK_COUNTER_BYTES, hipMemcpyDeviceToHost));
        for (int32_t v : h) if (v != 0) return 0;
        return 1;
    }
    return set_error(SMPLX_E_ARG, "no step has run on this stream");
}

int smplx_test_set_table_slots(smplx_space* s, int slots)
{
    if (!s || slots < 0 || (slots != 0 && (slots < 64 || (slots & (slots - 1)) != 0)))
        return set_error(SMPLX_E_ARG, "slots must be 0 or a power of two of at least 64");
    s->dt.test_slots = (size_t)slots;
    return SMPLX_OK;
}

long long smplx_test_table_slots(const smplx_space* s) { return s ? (long long)(s->dt.d_table ? s->dt.cap : 0) : -1; }

int smplx_test_table_probe(int nvars, int slots, int one_home, const int32_t* inserted, int n_inserted, const int32_t* queries, int n_queries,
                           int32_t* found_at_insert, int32_t* ids)
{
    if (!inserted || !queries || !found_at_insert || !ids || nvars < 1 || nvars > SMPLX_MAX_VARS || slots < 2 || slots > 4096 ||
        (slots & (slots - 1)) != 0 || n_inserted < 1 || n_inserted >= slots || n_queries < 1 || n_queries > 65536)
        return set_error(SMPLX_E_ARG, "bad argument (slots: a power of two up to 4096 with room for an empty slot)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return set_error(SMPLX_E_HIP, "no HIP device");
    const int stride = smplx_table_stride(nvars);
    DevBuf<int32_t> d_table, d_in, d_out;
    int e;
    const size_t n_max = (size_t)std::max(n_inserted, n_queries);
    if ((e = reserve(d_table, (size_t)slots * stride))) return e;
    if ((e = reserve(d_in, n_max * nvars))) return e;
    if ((e = reserve(d_out, n_max))) return e;
    HIP_TRY(hipMemset(d_table.p, 0, sizeof(int32_t) * (size_t)slots * stride));
    SmplxTableDev T;
    T.slots = d_table.p; T.mask = (uint32_t)(slots - 1); T.stride = stride; T.pad = 0;
    for (int pass = 0; pass < 2; ++pass) {     // the inserts, then the lookups in a launch of their own
        const int32_t* src = pass == 0 ? inserted : queries;
        const int n = pass == 0 ? n_inserted : n_queries;
        HIP_TRY(hipMemcpy(d_in.p, src, sizeof(int32_t) * (size_t)n * nvars, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_table_probe_ops, dim3(1), dim3(64), 0, 0, T, (const int*)d_in.p, n, nvars, one_home ? 1 : 0, pass == 0 ? 1 : 0, d_out.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(pass == 0 ? found_at_insert : ids, d_out.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    }
    return SMPLX_OK;
}

}  // extern "C"
