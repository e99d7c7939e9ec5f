// The k best candidates of one query, kept sorted by (d2, row) ascending: the list maintenance of csrc/grid_knn.hip ("v6q"; DESIGN.md section
// 4.26).  Plain C++ over an accessor, so that the kernel (entries in LDS) and a host program (tests/_knn_list_check.cpp, entries in an array)
// run the same text.  An accessor A has
//     double d2(int slot) const;   int row(int slot) const;   void set(int slot, double d2, int row);
// and the list's state is three values the caller keeps in registers: `fill` (entries held, 0 .. k) and, valid while fill == k, the worst
// entry (wd, wr) = slot k - 1.  A candidate that is not before the worst entry of a full list is rejected without touching the accessor.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KNN_LIST_HD __host__ __device__ __forceinline__
#else
#define KNN_LIST_HD inline
#endif

namespace knn_list {

// the order of the candidates: the smaller d2 first, among equal d2 the lower row
KNN_LIST_HD bool before(double da, int ra, double db, int rb) { return da < db || (da == db && ra < rb); }

struct State {
    int fill;
    double wd;
    int wr;
};

KNN_LIST_HD State empty() { return State{0, 0.0, 0}; }

// One candidate (d2, row) into a list of capacity k >= 1.  Not full: the entries behind the candidate's place move up one slot and the list
// grows.  Full: the worst entry falls off the end.  Entries equal in (d2, row) do not occur (a row is offered once).
template <class A>
KNN_LIST_HD void offer(A &a, int k, State &s, double d2, int row) {
    if (s.fill == k && !before(d2, row, s.wd, s.wr)) return;
    int p = s.fill < k ? s.fill : k - 1;                 // the slot that is free, or the one that is given up
    while (p > 0) {
        const double pd = a.d2(p - 1);
        const int pr = a.row(p - 1);
        if (!before(d2, row, pd, pr)) break;
        a.set(p, pd, pr);
        --p;
    }
    a.set(p, d2, row);
    if (s.fill < k) ++s.fill;
    if (s.fill == k) { s.wd = a.d2(k - 1); s.wr = a.row(k - 1); }
}

}  // namespace knn_list
