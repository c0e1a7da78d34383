// smpl_amd/csrc/device_table.h -- the device copy of the state table (K5; DeviceTable in space.h, SmplxTableDev in
// hs.table): allocation, growth at load factor 1/2, and the ride of the states committed since the last batch -- they
// wait in pending_ins and go up with the next frontier batch, or at once with table_flush.
#pragma once

#include <cstring>
#include <vector>

#include "kernels.h"
#include "space.h"

namespace {

int table_alloc(smplx_space* s, size_t cap)
{
    const int stride = smplx_table_stride(s->N);
    // the old table is freed first (the two need not fit side by side): if the new one cannot be had the space has none
    s->dt.cap = 0;
    s->hs.table.slots = nullptr;
    HIP_TRY(s->dt.d_table.alloc(cap * (size_t)stride));
    if (const hipError_t e = hipMemsetAsync(s->dt.d_table, 0, cap * (size_t)stride * sizeof(int32_t), s->stream)) {
        s->dt.d_table.reset();
        return hip_status(e, "table_alloc: hipMemsetAsync");
    }
    s->dt.cap = cap;
    s->hs.table.slots = s->dt.d_table;
    s->hs.table.mask = (uint32_t)(cap - 1);
    s->hs.table.stride = stride;
    s->hs.table.pad = 0;
    return SMPLX_OK;
}

// a new, empty device table of `cap` slots; every committed state is queued for the next upload
int table_realloc(smplx_space* s, size_t cap)
{
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (int e = table_alloc(s, cap)) return e;
    if (int e = upload_space(s)) return e;
    const int nstates = (int)s->lat.h_of_id.size();
    s->dt.pending_ins.clear();
    s->dt.pending_ins.reserve((size_t)nstates * (s->N + 2));
    for (int id = 1; id < nstates; ++id) {
        s->dt.pending_ins.push_back(0);
        s->dt.pending_ins.push_back(id);
        s->dt.pending_ins.insert(s->dt.pending_ins.end(), &s->lat.coords[(size_t)id * s->N], &s->lat.coords[(size_t)id * s->N] + s->N);
    }
    return SMPLX_OK;
}

// load factor above 1/2: a table four times the size, every committed state re-inserted with the next batch
int table_grow_if_needed(smplx_space* s)
{
    if (!s->dt.d_table || s->dt.count * 2 <= s->dt.cap) return SMPLX_OK;
    size_t cap = s->dt.cap;
    while (s->dt.count * 2 > cap) cap *= 4;
    ++s->dt.regrows;
    return table_realloc(s, cap);
}

// append the space's pending inserts to a staging array, tagged with its slot in the batch's query table
void table_take_pending(smplx_space* s, int slot, std::vector<int32_t>& items)
{
    const size_t w = (size_t)s->N + 2;
    const size_t o = items.size();
    items.insert(items.end(), s->dt.pending_ins.begin(), s->dt.pending_ins.end());
    for (size_t k = o; k < items.size(); k += w) items[k] = slot;
    s->dt.pending_ins.clear();
}

// upload staged inserts and run k_table_insert on `stream` (before the expansion kernels of the same stream)
int table_upload(smplx_space* lead, const std::vector<int32_t>& items, DevBuf<int32_t>& dbuf, PinBuf<int32_t>& pbuf, hipStream_t stream,
                 const SmplxSpaceDev* const* stab)
{
    if (items.empty()) return SMPLX_OK;
    const int n = (int)(items.size() / ((size_t)lead->N + 2));
    if (int e = reserve(dbuf, items.size())) return e;
    if (int e = reserve(pbuf, items.size())) return e;
    std::memcpy(pbuf.p, items.data(), items.size() * sizeof(int32_t));
    HIP_TRY(hipMemcpyAsync(dbuf.p, pbuf.p, items.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_table_insert, dim3(blocks_for(n, SMPLX_BLOCK)), dim3(SMPLX_BLOCK), 0, stream, lead->d_space, stab, dbuf.p, n, lead->N);
    HIP_TRY(hipGetLastError());
    return SMPLX_OK;
}

// first use of the device table on a space that was created without one (smplx_table_sync, the K5 entry points):
// allocate it for the states there are and queue them all
int table_ensure(smplx_space* s)
{
    if (s->dt.d_table) return SMPLX_OK;
    size_t cap = s->dt.test_slots ? s->dt.test_slots : (size_t)1 << 18;   // (test hook: a table small enough to be dense)
    const size_t nstates = s->lat.h_of_id.size();
    while (nstates * 2 > cap) cap *= 4;
    if (int e = table_realloc(s, cap)) return e;
    s->dt.count = nstates > 0 ? nstates - 1 : 0;
    return SMPLX_OK;
}

// the space's own batches: everything pending goes up on its stream
int table_flush(smplx_space* s, hipStream_t stream)
{
    if (!s->dt.d_table) return SMPLX_OK;
    if (int e = table_grow_if_needed(s)) return e;
    if (s->dt.pending_ins.empty()) return SMPLX_OK;
    std::vector<int32_t> items;
    table_take_pending(s, 0, items);
    return table_upload(s, items, s->dt.b_ins, s->dt.p_ins, stream, nullptr);
}

}  // namespace
