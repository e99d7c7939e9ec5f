// Stand-alone host program over csrc/knn_list.h (tests/test_grid_knn_oracle.py compiles it with AddressSanitizer and UndefinedBehaviorSanitizer).
// argv[1]: a file of float64 values, the d2 of a stream of candidates whose rows are given by argv[2] ("up": row = position in the stream,
// "down": row = length - 1 - position, "mix": row = (position * 7919) % length, a permutation for the prime lengths the test uses).  For each K in
// {8, 16, 32} and each capacity k in {1, K / 2 + 1, K} the stream is offered to a list held in an array of exactly k entries (an access past
// the list is an error of the address sanitizer), and the list is compared after EVERY offer with the first k of the sorted prefix.  Prints
// "ok <number of comparisons>" or the first difference.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>

#include "knn_list.h"

struct ArrayList {
    double *d;
    int *r;
    double d2(int s) const { return d[s]; }
    int row(int s) const { return r[s]; }
    void set(int s, double v, int j) { d[s] = v; r[s] = j; }
};

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s stream up|down|mix\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<double> v;
    double x;
    while (fread(&x, sizeof(double), 1, f) == 1) v.push_back(x);
    fclose(f);
    const int n = (int)v.size();
    std::vector<int> rows(n);
    for (int i = 0; i < n; ++i)
        rows[i] = !strcmp(argv[2], "up") ? i : (!strcmp(argv[2], "down") ? n - 1 - i : (int)(((long long)i * 7919) % n));
    long long checks = 0;
    for (int K : {8, 16, 32})
        for (int k : {1, K / 2 + 1, K}) {
            std::unique_ptr<double[]> d(new double[k]);           // exactly k entries on the heap: the sanitizer guards both ends
            std::unique_ptr<int[]> r(new int[k]);
            ArrayList a{d.get(), r.get()};
            knn_list::State s = knn_list::empty();
            std::vector<std::pair<double, int>> ref;
            for (int i = 0; i < n; ++i) {
                knn_list::offer(a, k, s, v[i], rows[i]);
                ref.insert(std::upper_bound(ref.begin(), ref.end(), std::make_pair(v[i], rows[i])), std::make_pair(v[i], rows[i]));
                const int want = std::min(k, (int)ref.size());
                if (s.fill != want) { printf("K %d k %d offer %d: fill %d, want %d\n", K, k, i, s.fill, want); return 1; }
                for (int t = 0; t < want; ++t, ++checks)
                    if (a.d2(t) != ref[t].first || a.row(t) != ref[t].second) {
                        printf("K %d k %d offer %d slot %d: (%.17g, %d), want (%.17g, %d)\n", K, k, i, t, a.d2(t), a.row(t), ref[t].first, ref[t].second);
                        return 1;
                    }
                if (s.fill == k && (s.wd != ref[k - 1].first || s.wr != ref[k - 1].second)) { printf("K %d k %d offer %d: stale worst entry\n", K, k, i); return 1; }
            }
        }
    printf("ok %lld\n", checks);
    return 0;
}
