// The star of one point of a view's Delaunay triangulation: what csrc/delaunay.hip's two kernels and its host twin share, so that
// the twin and the device take every decision by the same expressions in the same order.  Plain C++ over plain structs.
//
// The star of p is the cyclic list of its Delaunay neighbours among the points OFFERED so far, counter-clockwise around p.  A
// consecutive pair (a, b) is a finite vertex of p's cell if orient(p, a, b) > 0 and the gap (p is on the hull of what was offered;
// there is at most one, and the star keeps its index) otherwise.  Offering q keeps that invariant (include/mom4d.h has the rule); a point that was refused
// stays refused whatever is offered later, so the order of the offers decides no result, only which predicates are evaluated --
// and that order is fixed: cells row by row, a cell's points by index.
//
// Buckets are the image's pixel cells: cell (X, Y) holds the points with floor(u) = X, floor(v) = Y.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define DL_FN __host__ __device__ __forceinline__
#else
#define DL_FN inline
#endif

namespace dl {

struct P2 { double x, y; };

constexpr double kEps = 1.1102230246251565e-16;                 // 2^-53
constexpr double kOrientBound = (3.0 + 16.0 * kEps) * kEps;     // Shewchuk's first-stage bounds
constexpr double kCircleBound = (10.0 + 96.0 * kEps) * kEps;
constexpr double kGrow = 1.0 / 1048576.0;                       // circles and half-planes are grown by 2^-20 (relative and absolute)
constexpr double kThin = 1.0 / 1048576.0;                       // a vertex with |det| <= 2^-20 (|l| + |r|): its circle is not trusted
constexpr int kLaneRings = 3;                                   // the lane path gives up after the ring at this distance

enum { kDone = 0, kDefer = 1, kUncertain = -2, kOverflow = -3 };

// sign of orient(a, b, c): +1 counter-clockwise, -1 clockwise, 0 inside the filter bound
DL_FN int orient(P2 a, P2 b, P2 c)
{
#pragma clang fp contract(off)
    const double l = (a.x - c.x) * (b.y - c.y), r = (a.y - c.y) * (b.x - c.x), det = l - r;
    const double bound = kOrientBound * (fabs(l) + fabs(r));
    return det > bound ? 1 : (-det > bound ? -1 : 0);
}

// sign of incircle(a, b, c, d): +1 if d is inside the circle through the counter-clockwise a, b, c; 0 inside the filter bound
DL_FN int incircle(P2 a, P2 b, P2 c, P2 d)
{
#pragma clang fp contract(off)
    const double adx = a.x - d.x, ady = a.y - d.y, bdx = b.x - d.x, bdy = b.y - d.y, cdx = c.x - d.x, cdy = c.y - d.y;
    const double alift = adx * adx + ady * ady, blift = bdx * bdx + bdy * bdy, clift = cdx * cdx + cdy * cdy;
    const double bc1 = bdx * cdy, bc2 = bdy * cdx, ca1 = cdx * ady, ca2 = cdy * adx, ab1 = adx * bdy, ab2 = ady * bdx;
    const double det = alift * (bc1 - bc2) + blift * (ca1 - ca2) + clift * (ab1 - ab2);
    const double perm = alift * (fabs(bc1) + fabs(bc2)) + blift * (fabs(ca1) + fabs(ca2)) + clift * (fabs(ab1) + fabs(ab2));
    const double bound = kCircleBound * perm;
    return det > bound ? 1 : (-det > bound ? -1 : 0);
}

// One view: points (local indices), the cells' offsets [H W + 1] into cell_pts [n] (a cell's points ascending by index).
struct View {
    const P2* pts;
    const int* cell_start;
    const int* cell_pts;
    int n, H, W;
};

// The star: element i is s[i * stride] (the lane path interleaves the lanes of a workgroup in LDS).  Pair i is (S_i, S_i+1), cyclic;
// gap: the index of the pair that is the gap, -1 when the cell is closed.
struct Star {
    int* s;
    int stride, cap, m, gap;
    DL_FN int get(int i) const { return s[(size_t)i * stride]; }
    DL_FN void set(int i, int v) { s[(size_t)i * stride] = v; }
    DL_FN int next(int i) const { return i + 1 < m ? i + 1 : 0; }
    DL_FN int prev(int i) const { return i > 0 ? i - 1 : m - 1; }
};

DL_FN void star_remove(Star& S, int i)
{
    for (int k = i; k + 1 < S.m; ++k) S.set(k, S.get(k + 1));
    --S.m;
}

// q behind element `pos`; returns q's index
DL_FN int star_insert(Star& S, int pos, int q)
{
    for (int k = S.m; k > pos + 1; --k) S.set(k, S.get(k - 1));
    S.set(pos + 1, q);
    ++S.m;
    return pos + 1;
}

// Offers q to p's star.  0: refused (or p itself, or a neighbour already); 1: inserted; kUncertain; kOverflow.
// q's bisector cuts the cell iff q lies inside the circle of a finite vertex or in the gap's wedge.  The vertices it cuts are a run
// of the cyclic list, so the in-circle tests alone place q in a closed cell: no orientation of (p, neighbour, q) is evaluated
// there, and three points in a line that form no triangle make nothing uncertain.  Only the gap asks for orientations, with its
// two ends: orient(p, a, q) > 0 or orient(p, q, b) > 0 puts q in the wedge.
DL_FN int offer(const View& v, int p, P2 P, Star& S, int q)
{
    if (q == p) return 0;
    const int m = S.m;
    for (int i = 0; i < m; ++i)
        if (S.get(i) == q) return 0;
    const P2 Q = v.pts[q];
    if (m == 0) {
        if (S.cap < 1) return kOverflow;
        S.set(0, q);
        S.m = 1;
        S.gap = 0;
        return 1;
    }
    // the first cut vertex, and the run around it (it does not pass the gap)
    int kc = -1;
    for (int k = 0; k < m && m >= 2; ++k) {
        if (k == S.gap) continue;
        const int c = incircle(P, v.pts[S.get(k)], v.pts[S.get(S.next(k))], Q);
        if (c == 0) return kUncertain;
        if (c > 0) { kc = k; break; }
    }
    int k1 = kc, k2 = kc, cut = kc >= 0 ? 1 : 0;
    if (kc >= 0) {
        for (int k = S.next(k2); k != S.gap && k != k1; k = S.next(k)) {
            const int c = incircle(P, v.pts[S.get(k)], v.pts[S.get(S.next(k))], Q);
            if (c == 0) return kUncertain;
            if (c < 0) break;
            k2 = k;
            ++cut;
        }
        for (int k = S.prev(k1); k != S.gap && k != k2; k = S.prev(k)) {
            const int c = incircle(P, v.pts[S.get(k)], v.pts[S.get(S.next(k))], Q);
            if (c == 0) return kUncertain;
            if (c < 0) break;
            k1 = k;
            ++cut;
        }
        if (S.gap < 0 && cut >= m) return kUncertain;          // every vertex of a closed cell cut: not a star
    }
    int oa = 0, ob = 0;
    if (S.gap >= 0 && (kc < 0 || S.next(k2) == S.gap || S.prev(k1) == S.gap)) {
        oa = orient(v.pts[S.get(S.gap)], Q, P);                // orient(p, a, q)
        if (oa == 0) return kUncertain;
        ob = -oa;                                              // one neighbour: a is b
        if (m >= 2) {
            ob = orient(Q, v.pts[S.get(S.next(S.gap))], P);    // orient(p, q, b)
            if (ob == 0) return kUncertain;
        }
    }
    const bool in_gap = oa > 0 || ob > 0;
    if (kc < 0 && !in_gap) return 0;
    if (!in_gap) {
        // q takes the place of the neighbours between the run's first and last pair
        if (cut == 1 && m >= S.cap) return kOverflow;
        int pos = k1;
        for (int t = 1; t < cut; ++t) {
            const int idx = pos + 1 < S.m ? pos + 1 : 0;
            star_remove(S, idx);
            if (idx < pos) --pos;
            if (S.gap > idx) --S.gap;
        }
        star_insert(S, pos, q);
        if (S.gap > pos) ++S.gap;
        return 1;
    }
    // q enters the gap behind a.  From there the neighbours on either side go while q's pair with them is finite -- a walk does
    // not start across a gap -- and the vertex beyond them is cut
    if (m >= S.cap) return kOverflow;
    int j = star_insert(S, S.gap, q);
    bool fa = oa > 0, fb = ob > 0;
    while (fa && S.m >= 3) {
        const int ib = S.prev(j), ic = S.prev(ib);
        const P2 C = v.pts[S.get(ic)];
        const int c = incircle(P, C, v.pts[S.get(ib)], Q);
        if (c == 0) return kUncertain;
        if (c < 0) break;
        star_remove(S, ib);
        if (ib < j) --j;
        const int o = orient(C, Q, P);                         // orient(p, c, q): q's new pair
        if (o == 0) return kUncertain;
        fa = o > 0;
    }
    while (fb && S.m >= 3) {
        const int ib = S.next(j), ic = S.next(ib);
        const P2 C = v.pts[S.get(ic)];
        const int c = incircle(P, v.pts[S.get(ib)], C, Q);
        if (c == 0) return kUncertain;
        if (c < 0) break;
        star_remove(S, ib);
        if (ib < j) --j;
        const int o = orient(Q, C, P);                         // orient(p, q, c)
        if (o == 0) return kUncertain;
        fb = o > 0;
    }
    S.gap = !fa ? S.prev(j) : (!fb ? j : -1);
    return 1;
}

// 0: offer(q) would refuse q with every predicate it evaluates certain -- then it evaluates exactly these; 1: it would insert q or
// meet an uncertain predicate, and offer itself has to decide.  Reads the star only.
DL_FN int probe(const View& v, int p, P2 P, const Star& S, int q)
{
    if (q == p) return 0;
    const int m = S.m;
    for (int i = 0; i < m; ++i)
        if (S.get(i) == q) return 0;
    if (m == 0) return 1;
    const P2 Q = v.pts[q];
    for (int k = 0; k < m && m >= 2; ++k) {
        if (k == S.gap) continue;
        if (incircle(P, v.pts[S.get(k)], v.pts[S.get(S.next(k))], Q) >= 0) return 1;
    }
    if (S.gap >= 0) {
        if (m < 2 || orient(v.pts[S.get(S.gap)], Q, P) >= 0) return 1;
        if (orient(Q, v.pts[S.get(S.next(S.gap))], P) >= 0) return 1;
    }
    return 0;
}

// Offers the points cell_pts[b .. e) in that order.  0 / 1 (something was inserted) / an error.
// Wave: the 64 lanes of a wave work on ONE star (every lane holds the same p and S, the star's memory is the wave's): each probes
// its own candidate, and the first candidate, in order, that probe does not refuse goes through offer on every lane alike; the
// candidates behind it are probed again against the new star.  Every candidate thus meets the star the serial loop shows it, and
// the predicates that can raise a status are evaluated by offer alone: the same decisions as the serial loop.
template <int Wave>
DL_FN int offer_slice(const View& v, int p, P2 P, Star& S, int b, int e)
{
    if (b < 0) b = 0;
    if (e > v.n) e = v.n;
    int any = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    if (Wave) {
        const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        for (int base = b; base < e; base += 64) {
            const int k = base + lane;
            int q = k < e ? v.cell_pts[k] : -1;
            if (q < 0 || q >= v.n) q = -1;
            for (int from = 0; from < 64;) {
                const int open = (q >= 0 && lane >= from) ? probe(v, p, P, S, q) : 0;
                const unsigned long long todo = __ballot(open);
                if (!todo) break;
                const int first = __ffsll((long long)todo) - 1;
                const int rc = offer(v, p, P, S, __shfl(q, first));
                if (rc < 0) return rc;
                any |= rc;
                from = first + 1;
            }
        }
        return any;
    }
#endif
    for (int k = b; k < e; ++k) {
        const int q = v.cell_pts[k];
        if (q < 0 || q >= v.n) continue;
        const int rc = offer(v, p, P, S, q);
        if (rc < 0) return rc;
        any |= rc;
    }
    return any;
}

// Circumcircle of (P, A, B), grown so that rounding can only add to it.  False: the vertex is too thin for its centre to be
// trusted (the caller then takes the whole image).  With |det| > 2^-20 (|l| + |r|) centre and radius are good to 2^-29 of the radius.
DL_FN bool circle_of(P2 P, P2 A, P2 B, double& cx, double& cy, double& rho)
{
#pragma clang fp contract(off)
    const double ax = A.x - P.x, ay = A.y - P.y, bx = B.x - P.x, by = B.y - P.y;
    const double l = ax * by, r = ay * bx, det = l - r;
    if (!(fabs(det) > kThin * (fabs(l) + fabs(r)))) return false;
    const double a2 = ax * ax + ay * ay, b2 = bx * bx + by * by, d = 2.0 * det;
    const double ux = (by * a2 - ay * b2) / d, uy = (ax * b2 - bx * a2) / d;
    const double rr = sqrt(ux * ux + uy * uy);
    if (!(rr < 1e300)) return false;
    cx = P.x + ux;
    cy = P.y + uy;
    rho = rr * (1.0 + kGrow) + kGrow;
    return true;
}

// a double already clamped to [lo, hi] -> int
DL_FN int clamp_int(double x, int lo, int hi)
{
    if (!(x >= (double)lo)) return lo;                         // a NaN lands here
    if (x > (double)hi) return hi;
    return (int)x;
}

// The columns [x0, x1] of cell row Y that can hold a point x with  dx (x.y - P.y) - dy (x.x - P.x) > 0  (left of the ray from P
// along (dx, dy)), conservatively; x0 > x1: none.
DL_FN void halfplane_row(P2 P, double dx, double dy, int Y, int W, int& x0, int& x1)
{
#pragma clang fp contract(off)
    x0 = 0;
    x1 = W - 1;
    const double ya = (double)Y - P.y, yb = (double)Y + 1.0 - P.y;
    if (dy == 0.0) {
        if (dx > 0.0 ? !(yb >= 0.0) : (dx < 0.0 ? !(ya <= 0.0) : false)) x1 = -1;
        return;
    }
    const double ta = dx * ya / dy, tb = dx * yb / dy;
    if (!(fabs(ta) < 1e300) || !(fabs(tb) < 1e300)) return;    // the whole row
    if (dy > 0.0) {                                            // x < P.x + max(ta, tb)
        const double t = fmax(ta, tb), lim = P.x + t + kGrow * (1.0 + fabs(t) + fabs(P.x));
        if (lim < 0.0) x1 = -1; else x1 = clamp_int(floor(lim), 0, W - 1);
    } else {                                                   // x > P.x + min(ta, tb)
        const double t = fmin(ta, tb), lim = P.x + t - kGrow * (1.0 + fabs(t) + fabs(P.x));
        if (lim > (double)W) x1 = -1; else x0 = clamp_int(floor(lim), 0, W - 1);
    }
}

// Offers the cells of row Y between columns x0 and x1, which lie in the image: cell by cell, a cell's points by index -- one slice
// of cell_pts, the cells being stored row by row.  0 / 1 (something was inserted) / an error.
template <int Wave>
DL_FN int offer_span(const View& v, int p, P2 P, Star& S, int Y, int x0, int x1)
{
    if (x0 > x1) return 0;
    const size_t c = (size_t)Y * v.W;
    return offer_slice<Wave>(v, p, P, S, v.cell_start[c + x0], v.cell_start[c + x1 + 1]);
}

// Offers what vertex k of the star (the pair S_k, S_k+1) has to be checked against: the cells its grown circumcircle meets, or,
// for the gap, the cells that meet the wedge -- the union of the half-plane left of the ray to S_k and the one right of the ray
// to S_k+1.  0: nothing was inserted, the vertex stands; 1: something was inserted -- the scan went on over the region it had
// worked out (for the gap a superset of what is left of the wedge), and the caller's next pass looks at the new star; an error.
template <int Wave>
DL_FN int check_vertex(const View& v, int p, P2 P, Star& S, int k)
{
#pragma clang fp contract(off)
    const int m = S.m;
    if (m < 2) {                                               // nothing bounds the cell yet: everything is a candidate
        int any = 0;
        for (int Y = 0; Y < v.H; ++Y) {
            const int rc = offer_span<Wave>(v, p, P, S, Y, 0, v.W - 1);
            if (rc < 0) return rc;
            any |= rc;
        }
        return any;
    }
    const P2 A = v.pts[S.get(k)], B = v.pts[S.get(k + 1 < m ? k + 1 : 0)];
    int any = 0;
    if (k != S.gap) {
        double cx, cy, rho;
        const bool round = circle_of(P, A, B, cx, cy, rho);
        const int y0 = round ? clamp_int(floor(cy - rho), 0, v.H - 1) : 0;
        const int y1 = round ? (cy + rho < 0.0 ? -1 : clamp_int(floor(cy + rho), 0, v.H - 1)) : v.H - 1;
        if (round && cy - rho > (double)v.H) return 0;
        for (int Y = y0; Y <= y1; ++Y) {
            int x0 = 0, x1 = v.W - 1;
            if (round) {
                const double dy = cy < (double)Y ? (double)Y - cy : (cy > (double)Y + 1.0 ? cy - ((double)Y + 1.0) : 0.0);
                if (dy > rho) continue;
                const double hw = sqrt(rho * rho - dy * dy);
                if (cx + hw < 0.0 || cx - hw > (double)v.W) continue;
                x0 = clamp_int(floor(cx - hw), 0, v.W - 1);
                x1 = clamp_int(floor(cx + hw), 0, v.W - 1);
            }
            const int rc = offer_span<Wave>(v, p, P, S, Y, x0, x1);
            if (rc < 0) return rc;
            any |= rc;
        }
        return any;
    }
    for (int Y = 0; Y < v.H; ++Y) {
        int a0, a1, b0, b1;
        halfplane_row(P, A.x - P.x, A.y - P.y, Y, v.W, a0, a1);
        halfplane_row(P, -(B.x - P.x), -(B.y - P.y), Y, v.W, b0, b1);
        if (a0 <= a1 && b0 <= b1 && b0 <= a1 + 1 && a0 <= b1 + 1) {       // the two spans touch: one span
            a0 = a0 < b0 ? a0 : b0;
            a1 = a1 > b1 ? a1 : b1;
            b1 = -1;
        }
        int rc = a0 <= a1 ? offer_span<Wave>(v, p, P, S, Y, a0, a1) : 0;
        if (rc < 0) return rc;
        any |= rc;
        rc = b0 <= b1 ? offer_span<Wave>(v, p, P, S, Y, b0, b1) : 0;
        if (rc < 0) return rc;
        any |= rc;
    }
    return any;
}

// After the ring at distance r every point within r of p has been offered.  1: the cell is closed and every vertex's circle lies
// within r of p, the star is final; 0: not yet; kUncertain.
DL_FN int closed_within(const View& v, P2 P, const Star& S, int r)
{
#pragma clang fp contract(off)
    const int m = S.m;
    if (m < 3 || S.gap >= 0) return 0;
    for (int k = 0; k < m; ++k) {
        const P2 A = v.pts[S.get(k)], B = v.pts[S.get(k + 1 < m ? k + 1 : 0)];
        double cx, cy, rho;
        if (!circle_of(P, A, B, cx, cy, rho) || 2.0 * rho > (double)r) return 0;
    }
    return 1;
}

// The star of point p of a view with n >= 3.  lane: give up (kDefer) instead of going past the rings or the capacity.
// kDone: S is final and *gap is the index of the pair that is the gap, -1 for a point inside the hull.
template <int Wave>
DL_FN int build_star(const View& v, int p, Star& S, bool lane, int* gap)
{
    const P2 P = v.pts[p];
    const int X0 = clamp_int(floor(P.x), 0, v.W - 1), Y0 = clamp_int(floor(P.y), 0, v.H - 1);
    S.m = 0;
    S.gap = -1;
    *gap = -1;
    bool final_ = false;
    for (int r = 0; r <= kLaneRings && !final_; ++r) {
        const int ya = Y0 - r, yb = Y0 + r, xa = X0 - r, xb = X0 + r;
        for (int Y = (ya < 0 ? 0 : ya); Y <= (yb > v.H - 1 ? v.H - 1 : yb); ++Y) {
            // the ring's top and bottom rows in full, of the rows between them the two end cells
            const bool full = Y == ya || Y == yb;
            const int xl = xa < 0 ? 0 : xa, xr = xb > v.W - 1 ? v.W - 1 : xb;
            int rc = full ? offer_span<Wave>(v, p, P, S, Y, xl, xr) : (xa >= 0 ? offer_span<Wave>(v, p, P, S, Y, xa, xa) : 0);
            if (rc >= 0 && !full && xb <= v.W - 1) rc = offer_span<Wave>(v, p, P, S, Y, xb, xb);
            if (rc < 0) return (lane && rc == kOverflow) ? kDefer : rc;
        }
        if (xa <= 0 && ya <= 0 && xb >= v.W - 1 && yb >= v.H - 1) { final_ = true; break; }      // the whole image has been offered
        const int rc = closed_within(v, P, S, r);
        if (rc < 0) return rc;
        if (rc == 1) final_ = true;
    }
    if (!final_) {
        if (lane) return kDefer;
        // every vertex against the cells it reaches, until a whole pass inserts nothing
        int rounds = 0;                                        // a point enters a star once: n + 1 passes at the most
        for (bool changed = true; changed;) {
            changed = false;
            if (++rounds > 2 * v.n + 2) return kUncertain;
            for (int k = 0; k < (S.m < 2 ? 1 : S.m);) {
                const int rc = check_vertex<Wave>(v, p, P, S, k);
                if (rc < 0) return rc;
                if (rc == 1) changed = true;                   // the star has changed: the next pass sees what it is now
                ++k;
            }
        }
    }
    *gap = S.gap;
    return kDone;
}

// How many triangles p writes: its finite vertices (a, b) with p < a and p < b.
DL_FN int upper_count(const Star& S, int p, int gap)
{
    int c = 0;
    for (int k = 0; k < S.m; ++k)
        if (k != gap && S.get(k) > p && S.get(k + 1 < S.m ? k + 1 : 0) > p) ++c;
    return c;
}

// p's triangles (p, a, b), ascending by a, at out[3 * slot]; limit: slots out may hold.
DL_FN void emit_star(const Star& S, int p, int gap, int* out, size_t first, size_t limit)
{
    for (int k = 0; k < S.m; ++k) {
        const int a = S.get(k), b = S.get(k + 1 < S.m ? k + 1 : 0);
        if (k == gap || a <= p || b <= p) continue;
        int rank = 0;
        for (int i = 0; i < S.m; ++i) {
            const int a2 = S.get(i), b2 = S.get(i + 1 < S.m ? i + 1 : 0);
            if (i != gap && a2 > p && b2 > p && a2 < a) ++rank;
        }
        const size_t t = first + (size_t)rank;
        if (t < limit) { out[3 * t] = p; out[3 * t + 1] = a; out[3 * t + 2] = b; }
    }
}

}  // namespace dl
