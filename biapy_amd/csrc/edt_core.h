// The one-dimensional pieces of the exact Euclidean distance transform, without (edt.hip) and with (edt_index.hip) the nearest source: where
// a voxel's run of equal keys starts and ends in a row, and the lower envelope of parabolas over one run of a column with its query.  Compiles
// for the device (edt_kernels.h) and for the host (scripts/edt_cpu_check.cpp runs the same code over whole small volumes against a brute-force
// minimum).
//
// RULE (include/biapy_amd.h): out(v) = 0 where key(v) == 0, else the least |u - v|^2 over the voxels u with key(u) != key(v); EDT_INF where
// there is none.  Separable: the row pass leaves g = the squared distance along the row to the nearest voxel of another key; a column pass
// replaces, for a voxel of key k at y, the value by the minimum over y' of (y - y')^2 + (key(y') == k ? g(y') : 0).  A same-key y' beyond a
// foreign voxel is dominated by that foreign voxel, so the candidates are the voxel's own run and the one foreign voxel on each side of it:
// one lower envelope per run.  Background runs are skipped.
//
// A metric `M` states the arithmetic: EdtInt (unit grid, exact: int32 values, 64-bit sums) or EdtF64 (a grid step w, fp64 throughout).
// The envelope's stack lives behind a policy `S` with put(q, pos, t, h) / get(q, pos, t, h); entry q is the q-th surviving site: its position,
// the first position t at which it is the best so far, and its height h.  A run of a column of n positions pushes at most n sites (the run
// and, where the column goes on, one foreign voxel on each side), so n entries per stack suffice.
//
// THE NEAREST SOURCE.  Binary keys: 0 = a source, 1 = any other voxel.  Every voxel also gets the linear index of the source that realises its
// value; among equally near sources the one with the smallest linear index, -1 where there is none.  The separable passes deliver exactly
// that when each of them resolves ties to the smaller position: the row pass prefers the left source, a column pass the smaller y' among
// equal costs - which the envelope does on the integer path, where push pops only a top that is strictly worse and first_better is the first
// position at which the later site is strictly better.  On the fp64 path costs that differ by rounding only may go either way.  A policy with
// `S::SITES` carries that index as a payload per site in two int members: `cur` - stored with the entry by the next put - and `top` - the
// payload of the entry the last put or get handed over, i.e. of the envelope's top.  A policy without has neither.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define EDT_HD __host__ __device__ __forceinline__
#define EDT_UNROLL _Pragma("unroll")
#else
#define EDT_HD inline
#define EDT_UNROLL
#endif

#define EDT_INF INT32_MAX                 // integer results: "no voxel of another key anywhere so far"; the float results carry +inf
constexpr int EDT_BATCH = 4;              // column positions loaded ahead of the envelope work (independent loads in flight per thread)
constexpr int64_t EDT_SQ_LIMIT = INT32_MAX;   // integer path: Z^2 + Y^2 + X^2 must stay below (every finite result then is < EDT_INF)

// ---- the row: runs of equal keys ----------------------------------------------------------------------------------------------------
// `bnd` holds one bit per position of a 64-wide chunk starting at `base`.  Forward sweep: bit l set = the key at base + l differs from its
// left neighbour's; the run of the position at `lane` starts at the highest such bit at or below the lane, or at `carry` (the last start
// seen in earlier chunks; 0 = the run reaches the row's first voxel and has no foreign voxel on its left).
EDT_HD int64_t edt_run_start(uint64_t bnd, int lane, int64_t base, int64_t carry) {
  const uint64_t m = bnd & (~0ull >> (63 - lane));
  return m ? base + 63 - __builtin_clzll(m) : carry;
}
// Backward sweep: bit l set = the key at base + l differs from its right neighbour's; the run ends at the lowest such bit at or above the
// lane, or at `carry` (X - 1 = the run reaches the row's last voxel).
EDT_HD int64_t edt_run_end(uint64_t bnd, int lane, int64_t base, int64_t carry) {
  const uint64_t m = bnd >> lane;
  return m ? base + lane + __builtin_ctzll(m) : carry;
}
// steps from x to the foreign voxel left of a run starting at `start` / right of a run ending at `end`; 0 = there is none
EDT_HD int64_t edt_left_steps(int64_t x, int64_t start) { return start > 0 ? x - start + 1 : 0; }
EDT_HD int64_t edt_right_steps(int64_t x, int64_t end, int64_t X) { return end < X - 1 ? end - x + 1 : 0; }
// dl / dr = those steps to the left / right (0 = none): the steps to the nearer of the two, the left one on a tie, and - the foreign voxel
// being a source, `at` the voxel's own linear index - the linear index of that source, -1 where the row has none
EDT_HD int64_t edt_row_steps(int64_t dl, int64_t dr) { return dl == 0 ? dr : (dr == 0 || dl <= dr ? dl : dr); }
EDT_HD int32_t edt_row_site(int64_t at, int64_t dl, int64_t dr) {
  if (dl != 0 && (dr == 0 || dl <= dr)) return (int32_t)(at - dl);
  return dr != 0 ? (int32_t)(at + dr) : -1;
}

// ---- the metrics --------------------------------------------------------------------------------------------------------------------
struct EdtInt {
  typedef int32_t val;      // a stored value: < EDT_INF when finite (the host refuses shapes whose diagonal could reach it)
  typedef int64_t wide;     // a candidate sum: (46340)^2 + a finite value passes 2^31
  static EDT_HD val inf() { return EDT_INF; }
  EDT_HD val steps(int64_t d) const { return (val)(d * d); }                                  // row pass: d <= 46340
  EDT_HD wide cost(int x, int u, val h) const { const int64_t d = (int64_t)x - u; return d * d + h; }
  static EDT_HD val narrow(wide c) { return (val)c; }                                          // a minimum: below EDT_INF
  // first position at which site (u, hu) is strictly better than site (i, hi), i < u; clamped to n.  cost_i(x) <= cost_u(x) <=> 2 x (u - i)
  // <= u^2 - i^2 + hu - hi.  The caller has established cost_i(t) <= cost_u(t) at some t >= 0, so the numerator is not negative and the
  // truncating division is the floor.
  EDT_HD int first_better(int i, val hi, int u, val hu, int n) const {
    const int64_t num = (int64_t)u * u - (int64_t)i * i + hu - hi;
    const int64_t w = num / (2 * (int64_t)(u - i)) + 1;
    return w < n ? (int)w : n;
  }
};

struct EdtF64 {
  typedef double val;
  typedef double wide;
  double w;                 // the grid step of the axis at hand
  static EDT_HD val inf() { return (double)INFINITY; }
  EDT_HD val steps(int64_t d) const { const double s = w * (double)d; return s * s; }
  EDT_HD wide cost(int x, int u, val h) const { const double d = w * (double)((int64_t)x - u); return d * d + h; }
  static EDT_HD val narrow(wide c) { return c; }
  // the crossing in its midpoint form x* = (i + u) / 2 + (hu - hi) / (2 w^2 (u - i)): the first term is exact, the second carries a relative
  // error of a few 2^-53 of ITS size, which is at most the distance from the crossing to the farther site - a position misjudged next to the
  // crossing therefore gets a cost within a few 2^-51 (relative) of the minimum
  EDT_HD int first_better(int i, val hi, int u, val hu, int n) const {
    const double du = (double)((int64_t)u - i);
    const double x = 0.5 * ((double)i + (double)u) + (hu - hi) / (2.0 * w * w * du);
    const double f = floor(x) + 1.0;
    return f < (double)n ? (f > 0.0 ? (int)f : 0) : n;
  }
};

// ---- the envelope of one run ----------------------------------------------------------------------------------------------------------
template <class M, class S> struct EdtEnvelope {
  typedef typename M::val val;
  const M& m;
  S& st;
  int n;                   // column length: positions t are clamped to it
  int q;                   // index of the top entry, -1 = empty
  int tp, tt;              // the top entry, kept in registers: position, first position it wins at
  val th;                  //                                   height

  EDT_HD EdtEnvelope(const M& m_, S& st_, int n_) : m(m_), st(st_), n(n_), q(-1), tp(0), tt(0), th(0) {}
  EDT_HD void reset() { q = -1; }
  EDT_HD void pop() {
    if (--q >= 0) st.get(q, tp, tt, th);
  }
  // site u (ascending) of height h joins the envelope of the run starting at lo.  At most q + 1 <= n pops.
  EDT_HD void push(int lo, int u, val h) {
    if (h == M::inf()) return;                                            // no parabola
    while (q >= 0 && m.cost(tt, tp, th) > m.cost(tt, u, h)) pop();        // the top loses where its own stretch begins: it wins nowhere
    int t = lo;
    if (q >= 0) {
      t = m.first_better(tp, th, u, h, n);                                // > tt: at tt the top is no worse, and u gains on it with every step
      if (t <= tt) t = tt < n ? tt + 1 : n;                               // (exact arithmetic never comes here; a rounded fp64 crossing may)
    }
    ++q;
    tp = u; tt = t; th = h;
    st.put(q, u, t, h);
  }
  // the values of the run [s, e], written from e down to s: write(x, value, tp) with tp the winning site's column position, -1 where there is
  // none.  Entries whose stretch begins beyond e never win inside the run; entry 0 begins at s.  While write runs, the winning site is the top
  // entry - what the last put or get of the policy handed over (edt_column reads a payload there).
  template <class W> EDT_HD void flush(int s, int e, W&& write) {
    while (q >= 0 && tt > e) pop();
    for (int x = e; x >= s; --x) {
      if (q < 0) { write(x, M::inf(), -1); continue; }
      write(x, M::narrow(m.cost(x, tp, th)), tp);
      while (q >= 0 && tt >= x) pop();                                    // the stretches that begin at x (or, all of them beyond e gone, later)
    }
  }
};

// ---- one column ---------------------------------------------------------------------------------------------------------------------
// key(i) / load(i): the key and the value so far at position i; store(i, v, payload): the new value and, with S::SITES, the payload of the
// site that realises it, -1 where the value is inf (and always without S::SITES, where no payload exists at run time).  site(i), asked with
// S::SITES only: the payload the pass before left at position i (at a source: its own linear index, which is why the two foreign voxels
// bounding a run need no lookup of their own).  In place is fine for the values and for the payloads alike: a position is loaded before
// anything at or beyond it is stored, and the sites travel in the stack.  write_bg: also store 0 at background positions (a pass whose
// output is not its input); otherwise they are never stored and keep value 0 and, as sources, their own index.  Keys may be labels (runs of
// equal nonzero keys) in either form; a payload then says nothing at a foreign voxel that is no source, so no caller combines the two.
struct EdtNoSite {
  EDT_HD int operator()(int) const { return -1; }
};

template <class M, class S, class KeyF, class LoadF, class StoreF, class SiteF = EdtNoSite>
EDT_HD void edt_column(const M& m, S& st, int n, KeyF&& key, LoadF&& load, StoreF&& store, bool write_bg, SiteF&& site = SiteF()) {
  typedef typename M::val val;
  EdtEnvelope<M, S> env(m, st, n);
  auto carry = [&](int p) {                                               // the payload of the site pushed next
    if constexpr (S::SITES) st.cur = p;
  };
  auto write = [&](int x, val v, int tp) {
    if constexpr (S::SITES) store(x, v, tp < 0 ? -1 : st.top);
    else store(x, v, -1);
  };
  int s = 0, kprev = 0, pprev = -1;
  for (int i0 = 0; i0 < n; i0 += EDT_BATCH) {
    int kk[EDT_BATCH], pp[EDT_BATCH];
    val ff[EDT_BATCH];
    EDT_UNROLL
    for (int j = 0; j < EDT_BATCH; ++j) {
      kk[j] = 0; ff[j] = 0; pp[j] = -1;
      if (j < n - i0) {
        kk[j] = key(i0 + j); ff[j] = load(i0 + j);
        if constexpr (S::SITES) pp[j] = site(i0 + j);
      }
    }
    EDT_UNROLL
    for (int j = 0; j < EDT_BATCH; ++j) {
      if (j >= n - i0) break;
      const int i = i0 + j, k = kk[j], p = pp[j];
      if (i > 0 && k != kprev) {                                          // a run ends at i - 1, another starts at i
        if (kprev != 0) { carry(p); env.push(s, i, 0); env.flush(s, i - 1, write); }   // the foreign voxel after the run
        s = i;
        env.reset();
        if (k != 0) { carry(pprev); env.push(s, i - 1, 0); }              // the foreign voxel before the run
      }
      if (k != 0) { carry(p); env.push(s, i, ff[j]); }
      else if (write_bg) store(i, (val)0, p);
      kprev = k; pprev = p;
    }
  }
  if (kprev != 0) env.flush(s, n - 1, write);
}
