// ec3d_recurrence.hpp — the scalar steps of BiCGSTAB with restart (src/solvers.f90:31-49), each stated ONCE.
//
// Pure functions of doubles: no device state, no pointers, no HIP types, so the kernels (ec3d_kernels.hip,
// k_mg_scalar in ec3d_outer.hip) and a plain C++ program (tests/support/recurrence_cases.cpp) compile the same
// text.  Every operation is one rounded IEEE operation, in the operand order written here (the library is built
// with -ffp-contract=off); a zero divisor gives inf or NaN as the expression gives it -- nothing is caught.
// The oracle does not include this header: it is the checker.
#ifndef EC3D_RECURRENCE_HPP
#define EC3D_RECURRENCE_HPP

#include <cmath>

#ifdef __HIPCC__
#define EC3D_HD __host__ __device__
#else
#define EC3D_HD
#endif

// alpha = rr0 / (AP.R0)   (src/solvers.f90:32)
EC3D_HD inline double ec3d_alpha(double rr0, double d1) { return rr0 / d1; }

struct Ec3dNorm { double norm; bool exit; }; // a norm and its exit test
// ||S|| and "IF (norm2(S)/Bnorm < tolerance)"   (src/solvers.f90:34); ss = S.S
EC3D_HD inline Ec3dNorm ec3d_snorm_step(double ss, double bnorm, double tol)
{
    const double snorm = std::sqrt(ss);
    return Ec3dNorm{snorm, snorm / bnorm < tol};
}

// omega = (AS.S) / (AS.AS)   (src/solvers.f90:40)
EC3D_HD inline double ec3d_omega(double d2, double d3) { return d2 / d3; }

// ||R|| and "IF ((norm2(R)/Bnorm) < tolerance) EXIT"   (src/solvers.f90:43); rr = R.R
EC3D_HD inline Ec3dNorm ec3d_rnorm_step(double rr, double bnorm, double tol)
{
    const double rnorm = std::sqrt(rr);
    return Ec3dNorm{rnorm, rnorm / bnorm < tol};
}

// behind the ||R|| test: beta, the restart rule and the next iteration's rr0
struct Ec3dBeta { double beta; bool restart; double rr0_next; };
// rr0_new = R.R0, rr0 = this iteration's R.R0, rr = R.R
EC3D_HD inline Ec3dBeta ec3d_beta_step(double alpha, double omega, double rr0_new, double rr0, double rr, double bnorm,
                                       double tol)
{
    const double beta = (alpha / omega) * rr0_new / rr0;  // src/solvers.f90:45
    const bool restart = std::fabs(rr0_new) / bnorm < tol;     // src/solvers.f90:47
    // src/solvers.f90:48 and :31: after a restart R0 = R, so the next R.R0 is R.R (in the same summation order)
    return Ec3dBeta{beta, restart, restart ? rr : rr0_new};
}

#endif
