// The lock-free find-and-hook step of the mesh's union-find (mesh_components.hip), written once for device and host: the
// kernel instantiates it with agent-scope atomics, a stand-alone multi-threaded host program (tools/mesh_link_tsan.cpp)
// instantiates it with the compiler's __atomic builtins and runs it under a thread sanitizer.
//
// Roots are chosen by rank, a fixed permutation of the vertex indices (Ops::before), not by the index itself: on a mesh
// whose numbering follows its geometry, hooking the larger index under the smaller builds chains as long as a row of the
// mesh before any walk can shorten them, while a scrambled order keeps the trees shallow.  The component's smallest index
// is found afterwards, per root.
//
// Invariants.  parent[v] is v or an ancestor of v, and ranks strictly fall along every path to a root: a hook writes a
// root of lower rank into a word that still holds its own index (compare-and-swap), and a shortening stores a value read
// further up the same walk, which is still an ancestor.  A word that no longer holds its own index never does again, so a
// shortening cannot undo a hook.  The root of a finished tree is therefore the vertex of lowest rank in its component,
// whatever the order in which the edges were taken.
//
// Nothing here waits: the only retry follows a failed compare-and-swap, which means another lane hooked that root, and it
// walks on from where it stands.  `budget` counts walk steps plus retries of one edge; a lane that runs out returns false.
#pragma once

#ifndef MC_HD
#define MC_HD inline
#endif

// The rank of a vertex: an odd multiplier is a bijection on 32 bits, so no two vertices tie.
MC_HD unsigned int mc_rank(int v) { return (unsigned int)v * 0x9E3779B1u; }

// Ops: static int load(int*), static void shorten(int*, int) (an atomic store), static bool hook(int* word, int expected,
// int desired) (compare-and-swap, true when it stored).
template <class Ops>
MC_HD int mc_find(int* parent, int v, int& budget) {
    int p = Ops::load(parent + v);
    while (p != v) {
        if (--budget < 0) return -1;
        const int g = Ops::load(parent + p);
        if (g != p) Ops::shorten(parent + v, g);           // path halving: v's grandparent, an ancestor of v
        v = p;
        p = g;
    }
    return v;
}

// Joins the components of a and b, both inside the array.  False when the budget ran out.
template <class Ops>
MC_HD bool mc_link(int* parent, int a, int b, int budget) {
    for (;;) {
        const int ra = mc_find<Ops>(parent, a, budget), rb = mc_find<Ops>(parent, b, budget);
        if (ra < 0 || rb < 0) return false;
        if (ra == rb) return true;
        const bool a_wins = mc_rank(ra) < mc_rank(rb);
        const int loser = a_wins ? rb : ra, winner = a_wins ? ra : rb;
        if (Ops::hook(parent + loser, loser, winner)) return true;   // under the root of lower rank, while it is still a root
        if (--budget < 0) return false;
        a = loser;                                         // someone else hooked it: walk on from the two old roots
        b = winner;
    }
}
