// ec3d_outer.hpp — the outer iteration (ec3d_outer.hip) as its users ec3d_mg.hip and ec3d_null.hip see it: one
// description of a run's vectors (OuterRun), its start (ec3d_launch_begin for a solve, ec3d_outer_begin for an adjoint
// solve) and ec3d_outer_iteration, which takes what differs between users as callables.
#pragma once
#include "ec3d_stream.hpp"

#define EC3D_MG_DOT_BLOCKS 2048  // workgroups of the reducing kernels (grid-stride)

// ---- gating: every launch of iteration `it` is a no-op once the solve has stopped before it (strict = 0) or at it
// (strict = 1: the launches behind the ||S|| exit's check).  st == nullptr: not inside a solve (ec3d_precond_apply).
struct Gate {
    const SolverState *st;
    int it, strict;
};
__device__ __forceinline__ bool gated_off(const Gate &g)
{
    if (!g.st) return false;
    const int s = g.st->stop_iter; // written by an earlier launch on the stream: an ordinary load sees it
    return g.strict ? s <= g.it : s < g.it;
}
__device__ __forceinline__ void mg_stop_publish(SolverState *st, int it, int kind)
{
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(&st->stop_iter),
                       (unsigned long long)(unsigned)it | ((unsigned long long)(unsigned)kind << 32), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

inline unsigned blocks_of(int64_t n, int t = 256) { return (unsigned)((n + t - 1) / t); }
inline unsigned dot_blocks(int64_t n) { return (unsigned)std::min<int64_t>(EC3D_MG_DOT_BLOCKS, std::max<int64_t>(1, blocks_of(n))); }

// The vectors of one run, rows [0, n) of each
struct OuterRun {
    int64_t n;
    double *x, *r, *r0, *p, *v, *s, *t; // v = Op p^, t = Op s^
    void *ph, *sh;    // p^ = M p, s^ = M s: doubles, or floats that the kernels widen on load (f32); M = I: p and s
    bool f32;
    double *part;     // 2 * dot_blocks(n) doubles
    MgScalars *scal;
    double *hist;     // the residual history of a solve (c->hist, c->hist_cap); null and 0: none is written
    int64_t hist_cap;
};

// x = 0, r0 = p = r (k.r holds the right-hand side) and the state (c->state) of a run whose exits, restart rule and
// tolerance are the solve's own (ec3d_recurrence.hpp)
int ec3d_outer_begin(ec3d_ctx *c, const OuterRun &k, double tol);
// the launches of iteration `it` behind v = Op p^ (half 0: alpha, s, the ||s|| exit) and behind t = Op s^ (half 1:
// omega, x and r, the ||r|| exit, beta, p or the restart).  dotted: the operator's launch left the partials of r0.v
// (half 0) or of s.t and t.t (half 1) itself; otherwise a launch of k_avmg_dot makes them first.
void ec3d_outer_behind(ec3d_ctx *c, const OuterRun &k, int it, int half, bool dotted);

// One iteration: cycle(g, r, z) enqueues z = M r, op(g, x, a, y, two) y = Op x.  a and two are the dot that goes with
// the product, for an operator that sums it in its own launch (dotted); any other ignores them and its gate.
template <class Cycle, class Op>
inline void ec3d_outer_iteration(ec3d_ctx *c, const OuterRun &k, int it, bool dotted, const Cycle &cycle, const Op &op)
{
    const Gate g0{c->state, it, 0}, g1{c->state, it, 1};
    cycle(g0, k.p, k.ph);
    op(g0, k.ph, k.r0, k.v, 0);
    ec3d_outer_behind(c, k, it, 0, dotted);
    cycle(g1, k.s, k.sh);
    op(g1, k.sh, k.s, k.t, 1);
    ec3d_outer_behind(c, k, it, 1, dotted);
}

// ec3d_mg.hip: one iteration of an adjoint solve -- Op = A^T of the handle's matrix (ec3d_launch_spmv_t), M = N, the
// hierarchy of ec3d_null_mg_build whose p^ and s^ replace k's, or with m == nullptr M = I (k.ph = k.p, k.sh = k.s)
void ec3d_adjoint_iteration(ec3d_ctx *c, const ec3d_mg *m, const OuterRun &k, int it);
