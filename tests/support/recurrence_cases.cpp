// Stand-alone host program of tests/test_recurrence_host.py: calls the scalar steps of csrc/ec3d_recurrence.hpp and prints,
// per case, what it gave a function and what came back, every double as a hex float (%a):
//   KIND NAME : in ... : out ...
//   alpha : rr0 d1                              : alpha
//   snorm : ss bnorm tol                        : norm exit
//   omega : d2 d3                               : omega
//   rnorm : rr bnorm tol                        : norm exit
//   beta  : alpha omega rr0_new rr0 rr bnorm tol : beta restart rr0_next
// Reads nothing.  Built with -ffp-contract=off and the address and undefined-behaviour sanitizers.
#include "../../eddy_currents_3d_amd/csrc/ec3d_recurrence.hpp"

#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

namespace {

void p_alpha(const char *name, double rr0, double d1)
{
    std::printf("alpha %s : %a %a : %a\n", name, rr0, d1, ec3d_alpha(rr0, d1));
}
void p_omega(const char *name, double d2, double d3)
{
    std::printf("omega %s : %a %a : %a\n", name, d2, d3, ec3d_omega(d2, d3));
}
Ec3dNorm p_snorm(const char *name, double ss, double bnorm, double tol)
{
    const Ec3dNorm s = ec3d_snorm_step(ss, bnorm, tol);
    std::printf("snorm %s : %a %a %a : %a %d\n", name, ss, bnorm, tol, s.norm, (int)s.exit);
    return s;
}
Ec3dNorm p_rnorm(const char *name, double rr, double bnorm, double tol)
{
    const Ec3dNorm s = ec3d_rnorm_step(rr, bnorm, tol);
    std::printf("rnorm %s : %a %a %a : %a %d\n", name, rr, bnorm, tol, s.norm, (int)s.exit);
    return s;
}
Ec3dBeta p_beta(const char *name, double alpha, double omega, double rr0_new, double rr0, double rr, double bnorm, double tol)
{
    const Ec3dBeta b = ec3d_beta_step(alpha, omega, rr0_new, rr0, rr, bnorm, tol);
    std::printf("beta %s : %a %a %a %a %a %a %a : %a %d %a\n", name, alpha, omega, rr0_new, rr0, rr, bnorm, tol, b.beta,
                (int)b.restart, b.rr0_next);
    return b;
}

// ---- a real solve: BiCGSTAB with restart (the loop of the reference's sprsBCGstabWR, every scalar step through the header) on
// a nonsymmetric tridiagonal system of 48 unknowns
typedef std::vector<double> Vec;
Vec mul(const Vec &x)
{
    const size_t n = x.size();
    Vec y(n);
    for (size_t i = 0; i < n; ++i) {
        double s = 0.0;
        if (i > 0) s = s + -1.25 * x[i - 1];
        s = s + (2.5 + 0.01 * (double)i) * x[i];
        if (i + 1 < n) s = s + -0.75 * x[i + 1];
        y[i] = s;
    }
    return y;
}
double dot(const Vec &a, const Vec &b)
{
    double s = 0.0;
    for (size_t i = 0; i < a.size(); ++i) s = s + a[i] * b[i];
    return s;
}
void solve(double tol)
{
    const size_t n = 48;
    Vec b(n), x(n, 0.0);
    for (size_t i = 0; i < n; ++i) b[i] = 1.0 / (double)(i + 1) - 0.3;
    Vec r = mul(x);
    for (size_t i = 0; i < n; ++i) r[i] = b[i] - r[i];
    Vec r0 = r, p = r, s(n);
    const double bnorm = std::sqrt(dot(b, b));
    double rr0 = dot(r, r0);
    char name[32];
    for (int it = 1; it <= 200; ++it) {
        std::snprintf(name, sizeof name, "solve_it%d", it);
        const Vec ap = mul(p);
        const double d1 = dot(ap, r0);
        p_alpha(name, rr0, d1);
        const double alpha = ec3d_alpha(rr0, d1);
        for (size_t i = 0; i < n; ++i) s[i] = r[i] - alpha * ap[i];
        if (p_snorm(name, dot(s, s), bnorm, tol).exit) return;
        const Vec as = mul(s);
        const double d2 = dot(as, s), d3 = dot(as, as);
        p_omega(name, d2, d3);
        const double omega = ec3d_omega(d2, d3);
        for (size_t i = 0; i < n; ++i) r[i] = s[i] - omega * as[i];
        const double rr = dot(r, r), rr0_new = dot(r, r0);
        if (p_rnorm(name, rr, bnorm, tol).exit) return;
        const Ec3dBeta bs = p_beta(name, alpha, omega, rr0_new, rr0, rr, bnorm, tol);
        for (size_t i = 0; i < n; ++i) p[i] = r[i] + bs.beta * (p[i] - omega * ap[i]);
        if (bs.restart) {
            r0 = r;
            p = r;
        }
        rr0 = bs.rr0_next;
    }
}

} // namespace

int main()
{
    const double inf = std::numeric_limits<double>::infinity();
    solve(1e-10);

    // ---- each exit and the restart test at tol = the quotient itself and its two neighbours: `<`, not `<=`
    const double ss = 0x1.3c0ca428c59fbp-41, bnorm = 0x1.8b2e5f1a3c7d9p+3;
    {
        const double q = std::sqrt(ss) / bnorm;
        p_snorm("tol_below", ss, bnorm, std::nextafter(q, 0.0));
        p_snorm("tol_equal", ss, bnorm, q);
        p_snorm("tol_above", ss, bnorm, std::nextafter(q, inf));
        p_rnorm("tol_below", ss, bnorm, std::nextafter(q, 0.0));
        p_rnorm("tol_equal", ss, bnorm, q);
        p_rnorm("tol_above", ss, bnorm, std::nextafter(q, inf));
    }
    const double alpha = 0x1.91eb851eb851fp-2, omega = 0x1.3333333333333p-1, rr0 = 0x1.7a3c5e9d1b2f4p-19, rr = 0x1.02468ace13579p-38;
    for (int neg = 0; neg < 2; ++neg) { // the restart test takes |rr0_new|: the same three values for a negative rr0_new
        const double rr0_new = neg ? -0x1.5d2f8a6b4c3e1p-33 : 0x1.5d2f8a6b4c3e1p-33;
        const double q = std::fabs(rr0_new) / bnorm;
        p_beta(neg ? "neg_tol_below" : "tol_below", alpha, omega, rr0_new, rr0, rr, bnorm, std::nextafter(q, 0.0));
        p_beta(neg ? "neg_tol_equal" : "tol_equal", alpha, omega, rr0_new, rr0, rr, bnorm, q);
        p_beta(neg ? "neg_tol_above" : "tol_above", alpha, omega, rr0_new, rr0, rr, bnorm, std::nextafter(q, inf));
    }
    p_beta("neg_rr0_new", alpha, omega, -0x1.2p-10, rr0, rr, bnorm, 1e-10);

    // ---- zero divisors: inf and NaN come out as the expressions give them
    p_omega("d3_zero", 0x1.8p-3, 0.0);
    p_omega("d3_zero_neg", -0x1.8p-3, 0.0);
    p_omega("d2_d3_zero", 0.0, 0.0);
    p_alpha("d1_zero", rr0, 0.0);
    p_beta("omega_zero", alpha, 0.0, 0x1.2p-10, rr0, rr, bnorm, 1e-10);
    p_beta("omega_zero_rr0_new_zero", alpha, 0.0, 0.0, rr0, rr, bnorm, 1e-10); // inf * 0 = NaN; restart: 0 < tol
    p_beta("omega_inf", alpha, inf, 0x1.2p-10, rr0, rr, bnorm, 1e-10);
    p_beta("omega_nan", alpha, ec3d_omega(0.0, 0.0), 0x1.2p-10, rr0, rr, bnorm, 1e-10);
    p_beta("rr0_zero", alpha, omega, 0x1.2p-10, 0.0, rr, bnorm, 1e-10);

    // ---- rr == 0: ||R|| = 0 exits at any positive tol; a restart hands on rr = 0
    p_rnorm("rr_zero", 0.0, bnorm, 1e-10);
    p_rnorm("rr_zero_tol_zero", 0.0, bnorm, 0.0); // 0 < 0 is false
    p_snorm("ss_zero", 0.0, bnorm, 1e-10);
    p_beta("rr_zero_restart", alpha, omega, 0.0, rr0, 0.0, bnorm, 1e-10);
    p_snorm("bnorm_zero", ss, 0.0, 1e-10);       // inf < tol is false
    p_rnorm("rr_zero_bnorm_zero", 0.0, 0.0, 1e-10); // NaN < tol is false
    return 0;
}
