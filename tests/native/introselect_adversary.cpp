// Inputs that drive the MEDIAN selection of vslam_amd/csrc/introselect.h into its depth-limit fallback.
//
// The k-d build only ever asks for nth = n/2, and the median-of-3 killer of introselect_check.cpp never trips the depth limit
// of 2*floor(lg n) there.  McIlroy's adversary ("A Killer Adversary for Quicksort", 1999) does: items start as "gas" with no
// value, and the comparison function decides values lazily -- when two gas items meet, the one that was the last pivot
// candidate is frozen to the next solid value -- so every pivot the selection settles on turns out to be among the smallest of
// its range.  The item's identity travels in the key, `less` consults the adversary, and the gas left at the end gets distinct
// values above every solid one.  Frozen, the values are a fixed sequence of distinct floats that makes a plain run of the same
// algorithm take the same path: that sequence is what the device tests plant as x coordinates.
//
// usage: introselect_adversary n [n ...]
//   one line per n: "<n> <heap_select calls of the plain-float replay> <replay permutation == std::nth_element's> <key 0> ... <key n-1>"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

static int g_heap_calls = 0;
#define VS_SEL_ON_HEAP_SELECT() (++g_heap_calls)
#include "../../vslam_amd/csrc/introselect.h"

namespace {

constexpr int kGas = 1 << 30;

struct Adversary {
    std::vector<int> val;
    int nsolid = 0, candidate = -1;
    explicit Adversary(int n) : val((size_t)n, kGas) {}
    bool less(int x, int y) {
        if (val[x] == kGas && val[y] == kGas) val[x == candidate ? x : y] = nsolid++;
        if (val[x] == kGas) candidate = x;
        else if (val[y] == kGas) candidate = y;
        return val[x] < val[y];
    }
};

struct LazyStore {   // elements are item ids; the key IS the id, and its value is whatever the adversary has decided so far
    using value_type = int;
    using key_type = int;
    std::vector<int> *v;
    Adversary *adv;
    int key(int i) const { return (*v)[i]; }
    int key_of(const int &x) const { return x; }
    int get(int i) const { return (*v)[i]; }
    void set(int i, const int &x) { (*v)[i] = x; }
    void swap(int i, int j) { std::swap((*v)[i], (*v)[j]); }
    bool less(int a, int b) const { return adv->less(a, b); }
};

struct Item { float key; int id; };
struct FloatStore {
    using value_type = Item;
    using key_type = float;
    std::vector<Item> *v;
    float key(int i) const { return (*v)[i].key; }
    float key_of(const Item &x) const { return x.key; }
    Item get(int i) const { return (*v)[i]; }
    void set(int i, const Item &x) { (*v)[i] = x; }
    void swap(int i, int j) { std::swap((*v)[i], (*v)[j]); }
    bool less(float a, float b) const { return a < b; }
};

}  // namespace

int main(int argc, char **argv) {
    for (int a = 1; a < argc; a++) {
        const int n = atoi(argv[a]);
        if (n < 1 || n > (1 << 24)) return 2;   // the values must stay exact as floats
        std::vector<int> ids((size_t)n);
        for (int i = 0; i < n; i++) ids[i] = i;
        Adversary adv(n);
        LazyStore lazy{&ids, &adv};
        vs_sel::nth_element(lazy, 0, n / 2, n);
        for (int i = 0; i < n; i++)
            if (adv.val[i] == kGas) adv.val[i] = adv.nsolid++;

        std::vector<Item> base((size_t)n);
        for (int i = 0; i < n; i++) base[i] = Item{(float)adv.val[i], i};
        std::vector<Item> mine = base, theirs = base;
        g_heap_calls = 0;
        FloatStore fs{&mine};
        vs_sel::nth_element(fs, 0, n / 2, n);
        const int calls = g_heap_calls;
        std::nth_element(theirs.begin(), theirs.begin() + n / 2, theirs.end(),
                         [](const Item &x, const Item &y) { return x.key < y.key; });
        int same = 1;
        for (int i = 0; i < n; i++) same &= mine[i].id == theirs[i].id;

        printf("%d %d %d", n, calls, same);
        for (int i = 0; i < n; i++) printf(" %d", adv.val[i]);
        printf("\n");
    }
    return 0;
}
