// smpl_amd/csrc/model_lds.h -- the compiled model as the device code sees it, and the joint mathematics.
// Owns: the LDS address-space pointer types, ModelLds (the view of the LDS copy of the packed model, device_types.h
// SMPLX_BH_*) and ThreadLds (per-thread scratch in LDS, structure of arrays); the MV_* macros, which read per-variable
// data from the model-constants header in the per-robot build (SMPLX_CONST_MODEL, included here) and from LDS otherwise;
// xform .. apply_joint; as_global (SMPLX_GLOBAL_AS itself is in kernels.h); the staging of the model image into LDS
// (model_fetch, stage_model, setup_lds, setup_model_only).
// Restates: transform_functions.h:95-258 (joint transforms), robot_collision_state.h:419-421, 576 (chain step, sphere
// centre).
// BLOCK, the default thread count of a block, is defined by kernels.hip in front of its includes.
#pragma once

#ifndef __HIPCC_RTC__   // hiprtc (per-robot specialisation, specialize.cpp) brings its own runtime declarations
#include <hip/hip_runtime.h>
#endif

#include "det_math.h"
#include "device_types.h"
#include "kernels.h"

// ---------------------------------------------------------------------------------------------
// small helpers
// ---------------------------------------------------------------------------------------------

// LDS pointers are declared in address space 3: 32-bit, always lowered to ds_* instructions, half the
// scalar-register cost of generic pointers (the collision kernels are SGPR-bound).
#define LDS_AS __attribute__((address_space(3)))
typedef const LDS_AS SmplxJoint* JointPtr;
typedef const LDS_AS SmplxNode* NodePtr;
typedef const LDS_AS int* IntPtr;
typedef const LDS_AS double* DblPtr;

// The compiled model as the kernels see it: counts plus pointers into the LDS copy of the packed model
// (device_types.h SMPLX_BH_*).  Field names match SmplxModelDev so the device code reads the same either way.
struct ModelLds {
    int njoints, nvars, ntrees, nnodes, npairs, nslots, nroot;
    JointPtr joints;
    NodePtr nodes;
    IntPtr tree_first, tree_joint, tree_root_slot, pair_first, pair_other;
    DblPtr var_min, var_max, var_min_norm, var_k, coord_delta;
    IntPtr coord_vals, var_type;
    const SmplxBodiesDev* bodies;   // attached bodies of the query (HBM), null while it has none
};

struct ThreadLds {
    NodePtr nodes;            // shared: sphere trees
    LDS_AS double* d;         // per-thread doubles, SoA: d[e * BLOCK + tid]
    LDS_AS unsigned char* stk;   // per-thread byte stack, SoA
    int root_base;            // first double of root positions (3 per tree)
    int slot_base;            // first double of saved transforms (12 per slot)
    int q_base;               // first double of the configuration's joint values (one per planning variable)
    int stride;               // threads per block (SoA stride)
};

__device__ __forceinline__ LDS_AS double& lds_d(const ThreadLds& L, int e) { return L.d[e * L.stride + threadIdx.x]; }
__device__ __forceinline__ LDS_AS unsigned char& lds_b(const ThreadLds& L, int e) { return L.stk[e * L.stride + threadIdx.x]; }

// Per-variable model data.  In the per-robot build (SMPLX_CONST_MODEL) these are literals and the loops over the
// variables unroll; the generic kernels read the LDS copy of the model.
#ifdef SMPLX_CONST_MODEL
#include SMPLX_CONST_MODEL
#define MV_NVARS(M) CM_NV
#define ARG_NVARS(nvars) CM_NV     // the variable count where a kernel has it as an argument (index arithmetic in front of the model)
#define MV_TYPE(M, v) CM_VAR_TYPE[v]
#define MV_MIN(M, v) CM_VAR_MIN[v]
#define MV_MAX(M, v) CM_VAR_MAX[v]
#define MV_MIN_NORM(M, v) CM_VAR_MIN_NORM[v]
#define MV_K(M, v) CM_VAR_K[v]
#define MV_COORD_DELTA(M, v) CM_COORD_DELTA[v]
#define MV_COORD_VALS(M, v) CM_COORD_VALS[v]
#define MV_UNROLL _Pragma("unroll")
#else
#define MV_NVARS(M) (M)->nvars
#define ARG_NVARS(nvars) (nvars)
#define MV_TYPE(M, v) (M)->var_type[v]
#define MV_MIN(M, v) (M)->var_min[v]
#define MV_MAX(M, v) (M)->var_max[v]
#define MV_MIN_NORM(M, v) (M)->var_min_norm[v]
#define MV_K(M, v) (M)->var_k[v]
#define MV_COORD_DELTA(M, v) (M)->coord_delta[v]
#define MV_COORD_VALS(M, v) (M)->coord_vals[v]
#define MV_UNROLL
#endif

// p = T * c   (robot_collision_state.h:576); ((a*x + b*y) + c*z) + t
__device__ __forceinline__ void xform(const double T[12], const double c[3], double p[3])
{
    p[0] = ((T[0] * c[0] + T[1] * c[1]) + T[2] * c[2]) + T[3];
    p[1] = ((T[4] * c[0] + T[5] * c[1]) + T[6] * c[2]) + T[7];
    p[2] = ((T[8] * c[0] + T[9] * c[1]) + T[10] * c[2]) + T[11];
}

// local transform of a joint: origin * R(q)   (transform_functions.h:95-258)
__device__ __forceinline__ void joint_matrix(JointPtr j, double q, double J[12])
{
    DblPtr o = j->origin;
    const int kind = j->kind;
    if (kind == SMPLX_TK_FIXED) {
#pragma unroll
        for (int i = 0; i < 12; ++i) J[i] = o[i];
        return;
    }
    if (kind == SMPLX_TK_PRISMATIC) {   // translates along local Z whatever the axis (:218-226)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            J[4 * i + 0] = o[4 * i + 0]; J[4 * i + 1] = o[4 * i + 1]; J[4 * i + 2] = o[4 * i + 2];
            J[4 * i + 3] = ((o[4 * i + 0] * 0.0 + o[4 * i + 1] * 0.0) + o[4 * i + 2] * q) + o[4 * i + 3];
        }
        return;
    }
    double s, c;
    smplx_sincos(q, &s, &c);
    if (kind == SMPLX_TK_REV_X) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            J[4 * i + 0] = o[4 * i + 0];
            J[4 * i + 1] = c * o[4 * i + 1] + s * o[4 * i + 2];
            J[4 * i + 2] = c * o[4 * i + 2] - s * o[4 * i + 1];
            J[4 * i + 3] = o[4 * i + 3];
        }
    } else if (kind == SMPLX_TK_REV_Y) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            J[4 * i + 0] = c * o[4 * i + 0] - s * o[4 * i + 2];
            J[4 * i + 1] = o[4 * i + 1];
            J[4 * i + 2] = s * o[4 * i + 0] + c * o[4 * i + 2];
            J[4 * i + 3] = o[4 * i + 3];
        }
    } else if (kind == SMPLX_TK_REV_Z) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            J[4 * i + 0] = o[4 * i + 0] * c + o[4 * i + 1] * s;
            J[4 * i + 1] = o[4 * i + 1] * c - o[4 * i + 0] * s;
            J[4 * i + 2] = o[4 * i + 2];
            J[4 * i + 3] = o[4 * i + 3];
        }
    } else {   // generic axis: o * AngleAxis(q, axis)  (Eigen toRotationMatrix restated)
        const double ax = j->axis[0], ay = j->axis[1], az = j->axis[2];
        const double sx = s * ax, sy = s * ay, sz = s * az;
        const double c1 = 1.0 - c;
        const double cx = c1 * ax, cy = c1 * ay, cz = c1 * az;
        double R[9];
        double tmp;
        tmp = cx * ay; R[1] = tmp - sz; R[3] = tmp + sz;
        tmp = cx * az; R[2] = tmp + sy; R[6] = tmp - sy;
        tmp = cy * az; R[5] = tmp - sx; R[7] = tmp + sx;
        R[0] = cx * ax + c; R[4] = cy * ay + c; R[8] = cz * az + c;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                J[4 * i + k] = (o[4 * i + 0] * R[k] + o[4 * i + 1] * R[3 + k]) + o[4 * i + 2] * R[6 + k];
            J[4 * i + 3] = o[4 * i + 3];
        }
    }
}

// T = T * J   (robot_collision_state.h:419-421)
__device__ __forceinline__ void mul_affine(double T[12], const double J[12])
{
    double R[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            R[4 * i + k] = (T[4 * i + 0] * J[k] + T[4 * i + 1] * J[4 + k]) + T[4 * i + 2] * J[8 + k];
        R[4 * i + 3] = ((T[4 * i + 0] * J[3] + T[4 * i + 1] * J[7]) + T[4 * i + 2] * J[11]) + T[4 * i + 3];
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = R[i];
}

// the identity-origin forms (SMPLX_TK_*_T) with the origin's translation already in registers
__device__ __forceinline__ void apply_joint_t(int kind, double tx, double ty, double tz, double q, double T[12], bool on_root)
{
    if (on_root) {
#pragma unroll
        for (int i = 0; i < 12; ++i) T[i] = 0.0;
        T[0] = 1.0; T[5] = 1.0; T[10] = 1.0;
        T[3] = tx; T[7] = ty; T[11] = tz;
        if (kind == SMPLX_TK_FIXED_T) return;
        double s, c;
        smplx_sincos(q, &s, &c);
        if (kind == SMPLX_TK_REV_X_T) { T[5] = c; T[6] = 0.0 - s; T[9] = s; T[10] = c; }
        else if (kind == SMPLX_TK_REV_Y_T) { T[0] = c; T[2] = s; T[8] = 0.0 - s; T[10] = c; }
        else { T[0] = c; T[1] = 0.0 - s; T[4] = s; T[5] = c; }
        return;
    }
    // translation first: it uses the rotation of T before it is rotated
    const double n3 = ((T[0] * tx + T[1] * ty) + T[2] * tz) + T[3];
    const double n7 = ((T[4] * tx + T[5] * ty) + T[6] * tz) + T[7];
    const double n11 = ((T[8] * tx + T[9] * ty) + T[10] * tz) + T[11];
    T[3] = n3; T[7] = n7; T[11] = n11;
    if (kind == SMPLX_TK_FIXED_T) return;
    double s, c;
    smplx_sincos(q, &s, &c);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double a = T[4 * i + 0], b = T[4 * i + 1], d = T[4 * i + 2];
        if (kind == SMPLX_TK_REV_X_T) { T[4 * i + 1] = b * c + d * s; T[4 * i + 2] = d * c - b * s; }
        else if (kind == SMPLX_TK_REV_Y_T) { T[4 * i + 0] = a * c - d * s; T[4 * i + 2] = a * s + d * c; }
        else { T[4 * i + 0] = a * c + b * s; T[4 * i + 1] = b * c - a * s; }
    }
}

// One step of the kinematic chain: T = T * J(q), or T = J(q) for a joint on the root link.
// For origins whose rotation is exactly the identity (SMPLX_TK_*_T) the general form
//   J = origin * R_axis(q)   (transform_functions.h:104-207),   T' = T * J   (robot_collision_state.h:419-421)
// multiplies by 0 and 1 only; the terms x*1 and y*0 are exact, adding +-0 changes no non-zero value, and
// a*(-s) + b*c == b*c - a*s bit for bit, so the shortened expressions below give identical bits.
__device__ __forceinline__ void apply_joint(JointPtr jt, double q, double T[12], bool on_root)
{
    const int kind = jt->kind;
    if (kind < SMPLX_TK_FIXED_T) {
        double J[12];
        joint_matrix(jt, q, J);
        if (on_root) {
#pragma unroll
            for (int i = 0; i < 12; ++i) T[i] = J[i];
        } else {
            mul_affine(T, J);
        }
        return;
    }
    DblPtr o = jt->origin;
    apply_joint_t(kind, o[3], o[7], o[11], q, T, on_root);
}

// A pointer read out of a struct in memory (or out of LDS) is a FLAT address to the compiler: its loads and stores count on
// the LDS counter as well as on the memory counter, so every wait for an LDS read behind them waits for HBM too, and
// the other way round.  The buffers of this engine are all device memory: as_global says so.  (The type has to carry it: a
// cast to address space 1 and back is folded away, and the compiler takes no hint from an assumption.)
template <class T>
__device__ __forceinline__ SMPLX_GLOBAL_AS T* as_global(T* p) { return (SMPLX_GLOBAL_AS T*)p; }

// The first pieces of the packed model a thread copies (stage_model), in registers: all loads of a thread are issued
// before its first store.  A kernel that has the image and its size as arguments starts them at its very top, beside
// whatever else it reads first, and hands them to stage_model later.
typedef double __attribute__((ext_vector_type(2))) model_piece_t;
struct ModelFetch { model_piece_t v[4]; };
__device__ __forceinline__ ModelFetch model_fetch(const unsigned char* __restrict__ blob, int blob_bytes, int nthreads = BLOCK)
{
    const model_piece_t* src = reinterpret_cast<const model_piece_t*>(blob);
    const int total = blob_bytes / 16;
    ModelFetch f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + k * nthreads;
        if (i < total) f.v[k] = src[i];
    }
    return f;
}

// Cooperative copy of the packed model (a few KB) into LDS in 16-byte pieces; every later read of the model is a
// uniform-address LDS broadcast instead of a dependent global load.  Returns the view.
// blob, blob_bytes: the image (the space's model_blob) and its size; f: model_fetch(blob, blob_bytes, nthreads).  The
// header fields that become offsets are read from the image; the copy waits for none of them.
__device__ __forceinline__ ModelLds stage_model(const SmplxSpaceDev* __restrict__ S, unsigned char* smem, int nthreads,
                                                const unsigned char* __restrict__ blob, int blob_bytes, const ModelFetch& f)
{
    typedef model_piece_t d2_t;
    const int* hdr = reinterpret_cast<const int*>(blob);
    const d2_t* src = reinterpret_cast<const d2_t*>(blob);
    d2_t* dst = reinterpret_cast<d2_t*>(smem);
    const int total = blob_bytes / 16;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + k * nthreads;
        if (i < total) dst[i] = f.v[k];
    }
    for (int i = threadIdx.x + 4 * nthreads; i < total; i += nthreads) dst[i] = src[i];
    ModelLds M;
    M.njoints = hdr[SMPLX_BH_NJOINTS]; M.nvars = hdr[SMPLX_BH_NVARS]; M.ntrees = hdr[SMPLX_BH_NTREES];
    M.nnodes = hdr[SMPLX_BH_NNODES]; M.npairs = hdr[SMPLX_BH_NPAIRS]; M.nslots = hdr[SMPLX_BH_NSLOTS];
    M.nroot = hdr[SMPLX_BH_NROOT];
    LDS_AS unsigned char* base = (LDS_AS unsigned char*)smem;
    M.joints = (JointPtr)(base + hdr[SMPLX_BH_OFF_JOINTS]);
    M.nodes = (NodePtr)(base + hdr[SMPLX_BH_OFF_NODES]);
    IntPtr ip = (IntPtr)(base + hdr[SMPLX_BH_OFF_INTS]);
    M.tree_first = ip; ip += M.ntrees + 1;
    M.tree_joint = ip; ip += M.ntrees;
    M.tree_root_slot = ip; ip += M.ntrees;
    M.pair_first = ip; ip += M.ntrees + 1;
    M.pair_other = ip;
    DblPtr dp = (DblPtr)(base + hdr[SMPLX_BH_OFF_VARD]);
    M.var_min = dp; M.var_max = dp + M.nvars; M.var_min_norm = dp + 2 * M.nvars; M.var_k = dp + 3 * M.nvars;
    M.coord_delta = dp + 4 * M.nvars;
    IntPtr vp = (IntPtr)(base + hdr[SMPLX_BH_OFF_VARI]);
    M.coord_vals = vp; M.var_type = vp + M.nvars;
    M.bodies = S->bodies;
    return M;
}
// ... for a kernel that learns the size from the image's header
__device__ __forceinline__ ModelLds stage_model(const SmplxSpaceDev* __restrict__ S, unsigned char* smem, int nthreads = BLOCK)
{
    const int bytes = reinterpret_cast<const int*>(S->model_blob)[SMPLX_BH_BYTES];
    return stage_model(S, smem, nthreads, S->model_blob, bytes, model_fetch(S->model_blob, bytes, nthreads));
}

// model + per-thread scratch (root-position slots, saved transforms, DFS stack)
// (blob, blob_bytes, f: as stage_model)
__device__ __forceinline__ ThreadLds setup_lds(const SmplxSpaceDev* __restrict__ S, unsigned char* smem, ModelLds* Mv,
                                               int nthreads, bool slots_in_lds,
                                               const unsigned char* __restrict__ blob, int blob_bytes, const ModelFetch& f)
{
    ThreadLds L;
    *Mv = stage_model(S, smem, nthreads, blob, blob_bytes, f);
    L.stride = nthreads;
    L.nodes = Mv->nodes;
    L.d = (LDS_AS double*)((LDS_AS unsigned char*)smem + blob_bytes);
#ifdef SMPLX_CONST_MODEL
    const int nroot = 0;   // per-robot build: the root positions that lead a checked pair live in registers (ChainState::roots)
#else
    const int nroot = Mv->nroot;
#endif
    L.root_base = 0;
    L.slot_base = 3 * nroot;
    const int nslots = slots_in_lds ? Mv->nslots : 0;      // (a kernel that keeps the saved transforms in registers: const_chain<.., true>)
    L.q_base = 3 * nroot + 12 * nslots;
    const int nd = 3 * nroot + 12 * nslots + Mv->nvars;
    L.stk = (LDS_AS unsigned char*)(L.d + nd * nthreads);
    __syncthreads();
    return L;
}
__device__ __forceinline__ ThreadLds setup_lds(const SmplxSpaceDev* __restrict__ S, unsigned char* smem, ModelLds* Mv,
                                               int nthreads = BLOCK, bool slots_in_lds = true)
{
    const int bytes = reinterpret_cast<const int*>(S->model_blob)[SMPLX_BH_BYTES];
    return setup_lds(S, smem, Mv, nthreads, slots_in_lds, S->model_blob, bytes, model_fetch(S->model_blob, bytes, nthreads));
}

// kernels that only need the model (no per-thread scratch)
__device__ __forceinline__ ModelLds setup_model_only(const SmplxSpaceDev* __restrict__ S, unsigned char* smem, int nthreads = BLOCK)
{
#if defined(SMPLX_CONST_MODEL) && !CM_NEEDS_JOINTS
    // per-robot build: the planning-link chain and the per-variable data are literals, nothing is read from LDS
    ModelLds M = {};
    M.njoints = CM_NJ; M.nvars = CM_NV; M.ntrees = CM_NT;
    return M;
#else
    ModelLds M = stage_model(S, smem, nthreads);
    __syncthreads();
    return M;
#endif
}
