// smpl_amd/csrc/det_math.h -- deterministic double arithmetic shared by the host
// compiler (model_compile.cpp, g++) and the gfx950 kernels (hipcc).
//
// Arithmetic contract: every value that decides a
// discrete outcome on the path (a cell index, a waypoint count, a coordinate, a
// validity bit) is produced by the same sequence of IEEE-754 binary64
// +,-,*,/ and sqrt operations on the host and on the device.  Both compilers run
// with -ffp-contract=off, so no multiply-add is ever fused, and sin/cos are the
// fixed polynomial below instead of libm / ocml (whose last bits differ).
#pragma once

#ifndef __HIPCC_RTC__   // hiprtc (per-robot specialisation, specialize.cpp) brings its own runtime declarations
#include <math.h>
#endif

#if defined(__HIPCC__)
#define SMPLX_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SMPLX_HD inline
#endif

#define SMPLX_PI 3.14159265358979323846
#define SMPLX_2PI (2.0 * SMPLX_PI)

// sin(x), cos(x): 3-term Cody-Waite reduction by pi/2 + degree-13/14 minimax
// kernels on [-pi/4, pi/4].  Accuracy against the true value, measured with a 192-bit
// reference (tests/test_kinematics_ref.py holds it to 2.5 ulp or 2^-70): at most 1.4 ulp on
// [-pi, pi] and 2.2 ulp for |x| <= 1e5, 0.5 ulp for |x| <= 0.1.  Next to a zero of the
// function (x within a few doubles of a multiple of pi/2, |x| < 1e5) the reduction cancels:
// the absolute error stays below 2^-80 while the relative one reaches about 25 500 ulp of a
// result of about 1e-13.  Not correctly rounded anywhere; the contract is the same bits on
// host and device, not the last bit.
// Stands in for the reference's libm calls
// (sbpl_collision_checking/src/transform_functions.h:112-113,147-148,182-183;
//  smpl/src/graph/manip_lattice_action_space.cpp:591-594).
SMPLX_HD void smplx_sincos(double x, double* s_out, double* c_out)
{
    const double INVPIO2 = 6.36619772367581382433e-01;
    const double P1 = 0x1.921fb54400000p+0;
    const double P2 = 0x1.0b4611a600000p-34;
    const double P3 = 0x1.3198a2e000000p-69;
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03,
                 S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06,
                 S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03,
                 C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07,
                 C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
#ifdef ABL_NO_SINCOS
    *s_out = x * 0.5; *c_out = 1.0 - x * 0.25; return;
#endif
    const double fn = rint(x * INVPIO2);
    const int n = (int)fn;
    const double r = ((x - fn * P1) - fn * P2) - fn * P3;
    const double z = r * r;
    const double v = z * r;
    const double rs = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    const double ks = r + v * (S1 + z * rs);
    const double rc = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
    const double hz = 0.5 * z;
    const double w = 1.0 - hz;
    const double kc = w + (((1.0 - w) - hz) + z * rc);
    const int k = n & 3;
    *s_out = (k == 0) ? ks : (k == 1) ? kc : (k == 2) ? -ks : -kc;
    *c_out = (k == 0) ? kc : (k == 1) ? -ks : (k == 2) ? -kc : ks;
}

// acos(x) for x in [0, 1] (the argument is a clamped |cosine|; anything outside is the caller's to clamp): the
// rational approximation R(z) of (asin(t) - t) / t^3, z = t^2, on [0, 1/4] that the public fdlibm uses (e_acos.c).
//   x <  1/2: pi/2 - (x + x R(x^2)), pi/2 in two pieces
//   x >= 1/2: z = (1 - x) / 2, s = sqrt(z), acos = 2 (s + s R(z)); s is cut into a 26-bit head and its tail with a
//             Veltkamp split (a multiplication and two subtractions, no bit operations), so that head^2 is exact
// A fixed sequence of + - * / sqrt, the same bits on host and device.  Accuracy against the true value, measured over
// [0, 1] with the 192-bit reference of tests/kinematics_ref.py (tests/test_heuristics_host.py holds it to twice this):
// at most 0.77 ulp; exact at 0 (the double nearest pi/2) and at 1 (0).
// Stands in for std::acos in the reference's orientation distance (euclid_dist_heuristic.cpp:266).
SMPLX_HD double smplx_acos(double x)
{
    const double PIO2_HI = 1.57079632679489655800e+00, PIO2_LO = 6.12323399573676603587e-17;
    const double P0 = 1.66666666666666657415e-01, P1 = -3.25565818622400915405e-01, P2 = 2.01212532134862925881e-01,
                 P3 = -4.00555345006794114027e-02, P4 = 7.91534994289814532176e-04, P5 = 3.47933107596021167570e-05;
    const double Q1 = -2.40339491173441421878e+00, Q2 = 2.02094576023350569471e+00, Q3 = -6.88283971605453293030e-01,
                 Q4 = 7.70381505559019352791e-02;
    const bool low = x < 0.5;
    const double z = low ? x * x : (1.0 - x) * 0.5;
    const double p = z * (P0 + z * (P1 + z * (P2 + z * (P3 + z * (P4 + z * P5)))));
    const double q = 1.0 + z * (Q1 + z * (Q2 + z * (Q3 + z * Q4)));
    const double r = p / q;
    if (low) return PIO2_HI - (x - (PIO2_LO - x * r));
    const double s = sqrt(z);
    const double t = s * 134217729.0;          // 2^27 + 1
    const double df = t - (t - s);
    const double c = s > 0.0 ? (z - df * df) / (s + df) : 0.0;      // x = 1: 0 / 0 otherwise
    const double w = r * s + c;
    return 2.0 * (df + w);
}

// smpl/include/smpl/angles.h:45-62
SMPLX_HD double smplx_normalize_angle(double angle)
{
    if (fabs(angle) > SMPLX_2PI) angle = fmod(angle, SMPLX_2PI);
    if (angle < -SMPLX_PI) angle += SMPLX_2PI;
    if (angle > SMPLX_PI) angle -= SMPLX_2PI;
    return angle;
}

// smpl/include/smpl/angles.h:64-71
SMPLX_HD double smplx_normalize_angle_positive(double angle)
{
    angle = smplx_normalize_angle(angle);
    if (angle < 0.0) angle += SMPLX_2PI;
    return angle;
}

// smpl/include/smpl/angles.h:88-93
SMPLX_HD double smplx_shortest_angle_diff(double af, double ai) { return smplx_normalize_angle(af - ai); }
