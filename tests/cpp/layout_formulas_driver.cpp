// tests/cpp/layout_formulas_driver.cpp -- prints the engine's own layout formulas (device_types.h, kernels.h), one line
// per width and one per primitive count, for tests/test_width_references.py to hold its Python restatement to
#include <cstdio>

#include "../../smpl_amd/csrc/kernels.h"

int main()
{
    printf("limits %d %d %d %d\n", SMPLX_MAX_VARS, SMPLX_MAX_PRIMS, SMPLX_STEP_STATES, SMPLX_BLOCK);
    for (int nv = 1; nv <= SMPLX_MAX_VARS; ++nv) printf("nv %d %d %d\n", nv, smplx_table_stride(nv), smplx_rec_b_bytes(nv));
    for (int m = 4; m <= SMPLX_MAX_PRIMS; ++m)
        printf("M %d %d %d %d\n", m, smplx_small_block(m), smplx_search_block(m), smplx_step_states(m));
    return 0;
}
