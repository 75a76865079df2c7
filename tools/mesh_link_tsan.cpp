// Host check of the lock-free find-and-hook step (mvsnet_amd/csrc/mesh_link.h) under a thread sanitizer: eight threads link the
// edges of a permuted strip of 20 000 triangles and the roots are compared with a sequential union-find.
//   clang++ -O1 -g -fsanitize=thread -std=c++17 tools/mesh_link_tsan.cpp -o mesh_link_tsan -lpthread && ./mesh_link_tsan
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>
#include <algorithm>
#include "../mvsnet_amd/csrc/mesh_link.h"
struct HostOps {
    static int load(int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
    static void shorten(int* p, int v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }
    static bool hook(int* p, int e, int d) { return __atomic_compare_exchange_n(p, &e, d, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED); }
};
int main() {
    const int n = 20002, T = 8;
    std::vector<int> perm(n); for (int i = 0; i < n; ++i) perm[i] = i;
    srand(5); for (int i = n - 1; i > 0; --i) std::swap(perm[i], perm[rand() % (i + 1)]);
    std::vector<std::pair<int,int>> edges;
    for (int i = 0; i + 2 < n; ++i) { edges.push_back({perm[i], perm[i+1]}); edges.push_back({perm[i+1], perm[i+2]}); }
    for (int i = (int)edges.size() - 1; i > 0; --i) std::swap(edges[i], edges[rand() % (i + 1)]);
    std::vector<int> parent(n); for (int i = 0; i < n; ++i) parent[i] = i;
    std::atomic<int> bad{0};
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t) th.emplace_back([&, t] { for (size_t e = t; e < edges.size(); e += T) if (!mc_link<HostOps>(parent.data(), edges[e].first, edges[e].second, 1 << 22)) bad = 1; });
    for (auto& x : th) x.join();
    // sequential reference
    std::vector<int> ref(n); for (int i = 0; i < n; ++i) ref[i] = i;
    auto root = [&](std::vector<int>& p, int v) { while (p[v] != v) v = p[v]; return v; };
    for (auto& e : edges) { int a = root(ref, e.first), b = root(ref, e.second); if (a != b) { const bool aw = mc_rank(a) < mc_rank(b); ref[aw ? b : a] = aw ? a : b; } }
    int diff = 0, comps = 0;
    for (int i = 0; i < n; ++i) { diff += root(parent, i) != root(ref, i); comps += parent[i] == i; }
    printf("bad %d diff %d components %d\n", bad.load(), diff, comps);
    return bad || diff;
}
