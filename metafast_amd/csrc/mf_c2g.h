// mf_c2g.h -- what comp2graph (mf_comp2graph.hip, k <= 31) shares with its wide form (mf_wcomp2graph.hip, 32 <= k <= 63): the compacted
// de Bruijn graph of every component as GFA text, all components in one pass (ComponentsToGraph.java:70-130, Comp2Graph.java,
// GFAWriter.java).  Everything from the rows' flags to the text is here ONCE: c2g_build is the sequence of steps, the kernels that work on
// row, node and segment ids alone are plain kernels, and the three that read a k-mer -- k_c2g_segments, k_c2g_links_of,
// k_c2g_write_bases -- are templates over KEYS, the device's view of the rows' k-mers:
//
//   KEYS::kmer                         the k-mer's type (uint64_t / mf_u128: shifts, |, &, <, == are used on it as they are)
//   keys.oriented(node, k)             the k-mer of node 2 * row + strand as read on that strand
//   keys.last(node, k)                 its last base
//   KEYS::base(y, sh)                  the base at bit sh of y
//   KEYS::kmask(k) / revcomp(y, k)     4^k - 1; the reverse complement
//   keys.find(canonical, comp, &row)   the pair index: the row of (k-mer, component)
//
// and the host side hands c2g_build a SRC: n(), comp(), index(ctx, k) -- the pair index --, flags(ctx, A) -- the component-restricted neighbour pass into
// A.info / ridx / lidx / pal -- and get(), the KEYS (its type: SRC::keys).  The value pass over a sample's index differs with the table and stays with each tool.
//
//   k_c2g_links                        oriented nodes (2 * row + strand): f -> g iff g is the only right neighbour of f and f the only
//                                      left neighbour of g (Comp2Graph.mergePaths: both ends have ONE neighbour); never through a
//                                      palindromic k-mer (the reference holds it as two nodes with one sequence, so whoever touches it
//                                      sees two neighbours) and never f -> rc(f) (a hairpin: the reference merges a node with itself)
//   k_c2g_double                       pointer doubling towards the predecessors: head and distance of every node of a path, the
//                                      smallest node id of every cycle
//   k_c2g_ends / k_c2g_assign          of the two strands of a chain the one that starts on the smaller canonical k-mer; a cycle is
//                                      opened at its smallest canonical k-mer, on that k-mer's canonical strand; segment ids in
//                                      (component, paths by (canonical start k-mer, strand), then cycles) order from two scans
//   k_c2g_place / k_c2g_segments       rows in segment order, values scanned: KC; the printed strand (string order, A < C < G < T)
//   k_c2g_links_of<PASS>               per segment end the successors of its last k-mer -> link records, sorted as 64-bit keys
//   k_c2g_link_len / k_c2g_comp_base   line lengths, 64-bit scans, where a component's S and L lines start
//   k_c2g_write_s / _bases / _l        the text
//
// The grouped mf_ut_build is not the source of the segments: its emission rule (SequencesFinders: a path is printed from the end whose
// start k-mer is not above the k-mer the walk stopped ON or BEYOND, a palindromic start twice) prints some unitigs of a branching
// component twice and some never -- right for seq-builder's contigs, not for a graph whose every k-mer is drawn once.
#pragma once
#include <algorithm>
#include <errno.h>
#include <stdio.h>
#include <vector>
#include "mf_c2s.h"

#define C2G_NONE 0xFFFFFFFFu

struct mf_gfa {
    mf_ctx *ctx = nullptr;
    uint8_t *d_text = nullptr; size_t text_bytes = 0;
    uint64_t n_bytes = 0, n_segments = 0, n_links = 0, n_cycles = 0;
};

__device__ __forceinline__ uint32_t c2g_digits(uint64_t v) { uint32_t d = 1; while (v >= 10) { v /= 10; d++; } return d; }
// decimal, most significant digit first, at p; returns the digits written
__device__ __forceinline__ uint32_t c2g_put(uint8_t *p, uint64_t v) {
    const uint32_t d = c2g_digits(v);
    for (uint32_t i = d; i-- > 0;) { p[i] = (uint8_t)('0' + v % 10); v /= 10; }
    return d;
}
// code (A0 G1 C2 T3) -> place in the alphabet (A C G T): what String.compareTo orders by
__device__ __forceinline__ uint32_t c2g_rank(uint32_t c) { return c == 1u ? 2u : c == 2u ? 1u : c; }

// ---- links between oriented nodes ----
__device__ __forceinline__ bool c2g_l_unique(uint8_t info, uint32_t o) { return ((o ? info : (info >> 3)) & 7u) < 4u; }
static __global__ __launch_bounds__(256) void k_c2g_links(const uint8_t *__restrict__ info_, const uint32_t *__restrict__ ridx, const uint32_t *__restrict__ lidx,
                                                          const uint8_t *__restrict__ pal, uint64_t n, uint32_t *__restrict__ succ) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t info = info_[i];
    uint32_t s0 = C2G_NONE, s1 = C2G_NONE;
    if (!(pal && pal[i])) {
        if ((info & 7u) < 4u) {                              // x: right neighbour (ridx, ror)
            const uint32_t r = ridx[i], o = (info >> 6) & 1u;
            if (!(pal && pal[r]) && !(r == (uint32_t)i && o == 1u) && c2g_l_unique(info_[r], o)) s0 = 2u * r + o;
        }
        if (((info >> 3) & 7u) < 4u) {                       // rc(x): right neighbour = rc(left neighbour of x) = (lidx, !lor)
            const uint32_t l = lidx[i], o = ((info >> 7) & 1u) ^ 1u;
            if (!(pal && pal[l]) && !(l == (uint32_t)i && o == 0u) && c2g_l_unique(info_[l], o)) s1 = 2u * l + o;
        }
    }
    succ[2 * i] = s0; succ[2 * i + 1] = s1;
}
// the predecessor of f is the reverse complement of the successor of rc(f)
__device__ __forceinline__ uint32_t c2g_pred(const uint32_t *__restrict__ succ, uint32_t f) { const uint32_t g = succ[f ^ 1u]; return g == C2G_NONE ? C2G_NONE : (g ^ 1u); }

// word = pointer (low 32 bits) | distance << 32; a node without predecessor points at itself
static __global__ __launch_bounds__(256) void k_c2g_init(const uint32_t *__restrict__ succ, uint64_t nn, uint64_t *__restrict__ word, uint32_t *__restrict__ mn) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nn) return;
    const uint32_t p = c2g_pred(succ, (uint32_t)v);
    word[v] = (p == C2G_NONE || p == (uint32_t)v) ? v : ((uint64_t)p | (1ull << 32));
    mn[v] = (uint32_t)v;
}
// one round: a -> b.  *open counts the nodes whose pointer is not yet a node that points at itself (for ever so on a cycle)
static __global__ __launch_bounds__(256) void k_c2g_double(const uint64_t *__restrict__ wa, const uint32_t *__restrict__ ma, uint64_t nn, uint64_t *__restrict__ wb,
                                                    uint32_t *__restrict__ mb, unsigned int *__restrict__ open) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool still = false;
    if (v < nn) {
        const uint64_t a = wa[v];
        const uint32_t p = (uint32_t)a;
        const uint64_t b = wa[p];
        uint32_t m = ma[v];
        if ((uint32_t)b == p) wb[v] = a;
        else {
            wb[v] = (uint64_t)(uint32_t)b | ((uint64_t)((uint32_t)(a >> 32) + (uint32_t)(b >> 32)) << 32);
            const uint32_t m2 = ma[p];
            m = m2 < m ? m2 : m;
            still = true;
        }
        mb[v] = m;
    }
    const unsigned long long bal = __ballot(still);
    if (bal && mf_lane() == (uint32_t)(__ffsll((long long)bal) - 1)) atomicAdd(open, (unsigned int)__popcll(bal));
}

struct c2g_graph {
    const uint32_t *comp; const uint8_t *pal; const uint32_t *succ; const uint64_t *word; const uint32_t *mn;
    uint64_t n; int k;
};
// is v on a cycle?  Its pointer never became a node without predecessor
__device__ __forceinline__ bool c2g_on_cycle(const c2g_graph &G, uint32_t v, uint32_t *head, uint32_t *dist) {
    const uint64_t a = G.word[v];
    const uint32_t p = (uint32_t)a;
    *head = p; *dist = (uint32_t)(a >> 32);
    return (uint32_t)G.word[p] != p || c2g_pred(G.succ, p) != C2G_NONE;
}
// plen[s] = k-mers of the path that starts on node s, where s is the strand to print; clen[s] likewise for an opened cycle
static __global__ __launch_bounds__(256) void k_c2g_ends(c2g_graph G, uint32_t *__restrict__ plen, uint32_t *__restrict__ clen, unsigned int *__restrict__ n_cyc_rows) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * G.n) return;
    const uint32_t v = (uint32_t)t;
    if ((v & 1u) && G.pal && G.pal[v >> 1]) return;          // a palindromic k-mer is one node
    uint32_t h, d;
    if (c2g_on_cycle(G, v, &h, &d)) {
        if (G.mn[v] != v || (v & 1u)) return;                // opened at the smallest canonical k-mer, on its canonical strand
        uint32_t len = 1;
        for (uint32_t w = G.succ[v]; w != v; w = G.succ[w]) len++;
        clen[v] = len;
        atomicAdd(n_cyc_rows, len);
        return;
    }
    if (G.succ[v] != C2G_NONE) return;                       // v ends the path that h starts; its other strand runs from v ^ 1 to h ^ 1
    if ((h >> 1) < (v >> 1) || (h == v && !(v & 1u))) plen[h] = d + 1u;
}
static __global__ __launch_bounds__(256) void k_c2g_nonzero(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint64_t n, uint32_t *__restrict__ fa, uint32_t *__restrict__ fb) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { fa[i] = a[i] != 0u; fb[i] = b[i] != 0u; }
}
// off[c] = first row of component c (c = 0 .. nc)
static __global__ __launch_bounds__(256) void k_c2g_comp_off(const uint32_t *__restrict__ comp, uint64_t n, uint32_t nc, uint32_t *__restrict__ off) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = comp[i];
    if (i == 0) { for (uint32_t j = 0; j <= c; j++) off[j] = 0; }
    else { for (uint32_t j = comp[i - 1] + 1; j <= c; j++) off[j] = (uint32_t)i; }
    if (i == n - 1) for (uint32_t j = c + 1; j <= nc; j++) off[j] = (uint32_t)n;
}
struct c2g_segs {
    uint32_t *rseg, *rpos; uint8_t *ror;                     // per row: segment, place in it, strand of the row in it
    uint32_t *start, *len, *comp;                            // per segment: start node, k-mers, component
};
// segment ids: paths of component c from P[.] + (cycles of the components before c), its cycles after its paths
static __global__ __launch_bounds__(256) void k_c2g_assign(c2g_graph G, const uint32_t *__restrict__ plen, const uint32_t *__restrict__ clen, const uint64_t *__restrict__ P,
                                                    const uint64_t *__restrict__ Cy, const uint32_t *__restrict__ off, c2g_segs S) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * G.n) return;
    const uint32_t v = (uint32_t)t;
    if ((v & 1u) && G.pal && G.pal[v >> 1]) return;
    const uint32_t c = G.comp[v >> 1];
    uint32_t h, d;
    if (c2g_on_cycle(G, v, &h, &d)) {
        const uint32_t len = clen[v];
        if (!len) return;
        const uint32_t seg = (uint32_t)(P[2ull * off[c + 1]] + Cy[v]);
        S.start[seg] = v; S.len[seg] = len; S.comp[seg] = c;
        uint32_t w = v;
        for (uint32_t j = 0; j < len; j++) { S.rseg[w >> 1] = seg; S.rpos[w >> 1] = j; S.ror[w >> 1] = (uint8_t)(w & 1u); w = G.succ[w]; }
        return;
    }
    const uint32_t len = plen[h];
    if (!len) return;                                        // the other strand is the one
    const uint32_t seg = (uint32_t)(P[h] + Cy[2ull * off[c]]);
    S.rseg[v >> 1] = seg; S.rpos[v >> 1] = d; S.ror[v >> 1] = (uint8_t)(v & 1u);
    if (v == h) { S.start[seg] = v; S.len[seg] = len; S.comp[seg] = c; }
}
// rows in segment order: the node and the value at soff[segment] + place
static __global__ __launch_bounds__(256) void k_c2g_place(c2g_segs S, const uint64_t *__restrict__ soff, const uint32_t *__restrict__ val, uint64_t n, uint64_t n_seg,
                                                          uint32_t *__restrict__ nodeat, uint32_t *__restrict__ valat, unsigned int *__restrict__ flags) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint32_t seg = S.rseg[r];
    if ((uint64_t)seg >= n_seg || S.rpos[r] >= S.len[seg]) { atomicOr(flags, 8u); return; }      // (a row no segment took: rseg is C2G_NONE)
    const uint64_t at = soff[seg] + S.rpos[r];
    nodeat[at] = (uint32_t)(2 * r) + S.ror[r];
    valat[at] = val[r];
}
// base j of the segment as walked: the start k-mer's bases, then the last base of every further k-mer
template <class KEYS>
__device__ __forceinline__ uint32_t c2g_base(const KEYS &K, const uint32_t *__restrict__ nodeat, uint64_t so, typename KEYS::kmer y0, uint64_t j, int k) {
    if (j < (uint64_t)k) return KEYS::base(y0, 2 * (k - 1 - (int)j));
    return K.last(nodeat[so + j - (uint64_t)k + 1], k);
}
struct c2g_lines {
    uint8_t *cmp;            // per segment: 0 the walked strand is printed, 1 it equals its reverse complement, 2 the reverse complement is printed
    uint64_t *kc;            // KC
    uint32_t *slen;          // bytes of its S line(s)
};
__device__ __forceinline__ uint32_t c2g_name_len(uint32_t seg, uint32_t c, const uint64_t *__restrict__ segbase) {
    return c2g_digits((uint64_t)seg - segbase[c] + 1) + 2u + c2g_digits(c);
}
template <class KEYS>
static __global__ __launch_bounds__(256) void k_c2g_segments(KEYS K, c2g_graph G, c2g_segs S, uint64_t n_seg, const uint64_t *__restrict__ soff,
                                                             const uint32_t *__restrict__ nodeat, const uint32_t *__restrict__ valat, const uint64_t *__restrict__ vsum,
                                                             const uint64_t *__restrict__ segbase, c2g_lines L) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seg) return;
    const int k = G.k;
    const uint64_t so = soff[s], len = S.len[s], nb = len + (uint64_t)k - 1;
    const typename KEYS::kmer y0 = K.oriented(S.start[s], k);
    uint32_t cmp = 1;
    for (uint64_t j = 0; 2 * j < nb; j++) {                  // seq against its reverse complement, GFAWriter.java:33
        const uint32_t a = c2g_rank(c2g_base(K, nodeat, so, y0, j, k)), b = c2g_rank(3u - c2g_base(K, nodeat, so, y0, nb - 1 - j, k));
        if (a != b) { cmp = a < b ? 0u : 2u; break; }
    }
    L.cmp[s] = (uint8_t)cmp;
    // GFAWriter.java:66-71: every k-mer's value, and k - 1 times that of the printed strand's last k-mer
    const uint64_t kc = vsum[so + len] - vsum[so] + (uint64_t)(k - 1) * (uint64_t)valat[cmp == 2u ? so : so + len - 1];
    L.kc[s] = kc;
    const uint32_t line = 2u + c2g_name_len((uint32_t)s, S.comp[s], segbase) + 1u + (uint32_t)nb + 6u + c2g_digits(nb) + 6u + c2g_digits(kc) + 1u;
    L.slen[s] = cmp == 1u ? 2u * line : line;                // the reference prints a palindromic k-mer's node twice
}
static __global__ __launch_bounds__(256) void k_c2g_comp_base(const uint64_t *__restrict__ P, const uint64_t *__restrict__ Cy, const uint32_t *__restrict__ off, uint32_t nc,
                                                       uint64_t *__restrict__ segbase) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > nc) return;
    segbase[c] = P[2ull * off[c]] + Cy[2ull * off[c]];
}
// PASS 0: links per segment end; PASS 1: the records, key = from << 33 | from is '-' << 32 | to << 1 | to is '-'
template <int PASS, class KEYS>
static __global__ __launch_bounds__(256) void k_c2g_links_of(KEYS K, c2g_graph G, c2g_segs S, uint64_t n_seg, const uint64_t *__restrict__ soff,
                                                             const uint32_t *__restrict__ nodeat, const uint8_t *__restrict__ cmp, uint32_t *__restrict__ cnt,
                                                             const uint64_t *__restrict__ loff, uint64_t *__restrict__ rec, unsigned int *__restrict__ flags) {
    typedef typename KEYS::kmer kmer;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * n_seg) return;
    const uint64_t s = t >> 1;
    const uint32_t e = (uint32_t)t & 1u;                     // 0: the walked strand leaves through its last k-mer; 1: its reverse complement
    const int k = G.k;
    const kmer kmask = KEYS::kmask(k);
    const uint32_t c = S.comp[s], cs = cmp[s];
    const uint32_t endn = e ? (nodeat[soff[s]] ^ 1u) : nodeat[soff[s] + S.len[s] - 1];
    const kmer y = K.oriented(endn, k);
    const uint64_t fminus = e ? (cs >= 1u ? 0u : 1u) : (cs <= 1u ? 0u : 1u);      // printEdge: '+' when the strand that leaves is the printed one
    uint32_t m = 0;
    uint64_t at = PASS ? loff[t] : 0;
    for (uint32_t nuc = 0; nuc < 4; nuc++) {
        const kmer z = ((y << 2) | (kmer)nuc) & kmask, rz = KEYS::revcomp(z, k), cz = z < rz ? z : rz;
        uint32_t r;
        if (!K.find(cz, c, &r)) continue;
        const uint32_t to = S.rseg[r], tc = cmp[to], oz = cz != z, same = oz == S.ror[r];
        uint64_t tminus; uint32_t mult = 1;
        if (z == rz) { tminus = 0; mult = 2; }               // a palindromic k-mer: two nodes of the reference answer to it
        else if (same && S.rpos[r] == 0) tminus = tc <= 1u ? 0u : 1u;
        else if (!same && S.rpos[r] == S.len[to] - 1) tminus = tc >= 1u ? 0u : 1u;
        else { atomicOr(flags, 4u); continue; }              // (a successor inside a segment: the links and the flags disagree)
        if (PASS) { const uint64_t key = (s << 33) | (fminus << 32) | ((uint64_t)to << 1) | tminus; for (uint32_t j = 0; j < mult; j++) rec[at++] = key; }
        m += mult;
    }
    if (!PASS) cnt[t] = m;
}
static __global__ __launch_bounds__(256) void k_c2g_link_len(const uint64_t *__restrict__ rec, uint64_t n_links, const uint32_t *__restrict__ scomp, const uint64_t *__restrict__ segbase,
                                                             int k, uint32_t *__restrict__ llen) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_links) return;
    const uint64_t key = rec[i];
    const uint32_t from = (uint32_t)(key >> 33), to = (uint32_t)(key >> 1) & 0x7FFFFFFFu, c = scomp[from];
    llen[i] = 2u + c2g_name_len(from, c, segbase) + 3u + c2g_name_len(to, c, segbase) + 3u + c2g_digits((uint64_t)(k - 1)) + 2u;
}
// lbase[c] = first link record of component c (c = 0 .. nc): the records are sorted by segment
static __global__ __launch_bounds__(256) void k_c2g_link_base(const uint64_t *__restrict__ rec, uint64_t n_links, const uint64_t *__restrict__ segbase, uint32_t nc,
                                                       uint64_t *__restrict__ lbase) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > nc) return;
    const uint64_t want = segbase[c];
    uint64_t lo = 0, hi = n_links;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if ((rec[mid] >> 33) < want) lo = mid + 1; else hi = mid; }
    lbase[c] = lo;
}
struct c2g_text {
    const uint64_t *es, *el, *segbase, *lbase;               // scans of the S and L line lengths; per component: first segment, first link
    uint64_t *seqoff;                                        // per segment: where its bases start
    uint8_t *text;
};
// everything of an S line but the bases
static __global__ __launch_bounds__(256) void k_c2g_write_s(c2g_segs S, uint64_t n_seg, c2g_lines L, c2g_text T, int k) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seg) return;
    const uint32_t c = S.comp[s];
    const uint64_t nb = (uint64_t)S.len[s] + (uint64_t)k - 1;
    const uint32_t copies = L.cmp[s] == 1u ? 2u : 1u, line = L.slen[s] / copies;
    uint64_t at = T.es[s] + T.el[T.lbase[c]];
    for (uint32_t j = 0; j < copies; j++, at += line) {
        uint8_t *p = T.text + at;
        *p++ = 'S'; *p++ = '\t';
        p += c2g_put(p, s - T.segbase[c] + 1); *p++ = '_'; *p++ = 'i'; p += c2g_put(p, c); *p++ = '\t';
        if (j == 0) T.seqoff[s] = (uint64_t)(p - T.text);
        p += nb;
        *p++ = '\t'; *p++ = 'L'; *p++ = 'N'; *p++ = ':'; *p++ = 'i'; *p++ = ':'; p += c2g_put(p, nb);
        *p++ = '\t'; *p++ = 'K'; *p++ = 'C'; *p++ = ':'; *p++ = 'i'; *p++ = ':'; p += c2g_put(p, L.kc[s]);
        *p++ = '\n';
    }
}
// a row writes the last base of its k-mer; the first row of a segment the k - 1 bases before it as well
template <class KEYS>
static __global__ __launch_bounds__(256) void k_c2g_write_bases(KEYS K, c2g_graph G, c2g_segs S, c2g_lines L, c2g_text T) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= G.n) return;
    const int k = G.k;
    const uint32_t s = S.rseg[r], p = S.rpos[r], cs = L.cmp[s];
    const uint64_t nb = (uint64_t)S.len[s] + (uint64_t)k - 1;
    const typename KEYS::kmer y = K.oriented((uint32_t)(2 * r) + S.ror[r], k);
    uint8_t *q = T.text + T.seqoff[s];
    const uint32_t line = cs == 1u ? L.slen[s] / 2u : 0u;
    for (int j = p ? k - 1 : 0; j < k; j++) {
        const uint32_t b = KEYS::base(y, 2 * (k - 1 - j));
        const uint64_t at = (uint64_t)p + (uint64_t)j;
        if (cs == 2u) q[nb - 1 - at] = (uint8_t)"AGCT"[3u - b];
        else { q[at] = (uint8_t)"AGCT"[b]; if (line) q[at + line] = (uint8_t)"AGCT"[b]; }
    }
}
static __global__ __launch_bounds__(256) void k_c2g_write_l(const uint64_t *__restrict__ rec, uint64_t n_links, const uint32_t *__restrict__ scomp, c2g_text T, int k) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_links) return;
    const uint64_t key = rec[i];
    const uint32_t from = (uint32_t)(key >> 33), to = (uint32_t)(key >> 1) & 0x7FFFFFFFu, c = scomp[from];
    uint8_t *p = T.text + T.el[i] + T.es[T.segbase[c + 1]];
    *p++ = 'L'; *p++ = '\t';
    p += c2g_put(p, from - T.segbase[c] + 1); *p++ = '_'; *p++ = 'i'; p += c2g_put(p, c);
    *p++ = '\t'; *p++ = ((key >> 32) & 1ull) ? '-' : '+'; *p++ = '\t';
    p += c2g_put(p, to - T.segbase[c] + 1); *p++ = '_'; *p++ = 'i'; p += c2g_put(p, c);
    *p++ = '\t'; *p++ = (key & 1ull) ? '-' : '+'; *p++ = '\t';
    p += c2g_put(p, (uint64_t)(k - 1)); *p++ = 'M'; *p++ = '\n';
}

// ---- values per row ----
static __global__ __launch_bounds__(256) void k_c2g_fill(uint32_t *__restrict__ val, uint64_t n, uint32_t v) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) val[r] = v;
}
// the value a sample adds to a row that it holds with count cnt > 0: coverage = 0 adds 1, else the count, bounded as
// BigLong2ShortHashMap.addAndBound bounds
__device__ __forceinline__ uint32_t c2g_add_value(uint32_t v, uint32_t cnt, int coverage) {
    v += coverage ? cnt : 1u;
    return v > (uint32_t)MF_MAX_COUNT ? (uint32_t)MF_MAX_COUNT : v;
}

// ---------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------
// val = first (1 without samples: every member k-mer is worth 1; 0 with them)
static int c2g_values_first(mf_ctx *ctx, uint64_t n_rows, uint32_t first, mf_buf<uint32_t> &val) {
    MF_TRY(val.alloc(ctx, n_rows));
    if (n_rows) {
        mf_ktimer tm(ctx, "k_c2g_values");
        k_c2g_fill<<<c2s_grid(n_rows), 256, 0, ctx->stream>>>(val.p, n_rows, first);
    }
    return MF_OK;
}

// rows + values -> the text.  SRC: the rows of one width (c2g_narrow_rows, mf_comp2graph.hip; c2g_wide_rows, mf_wcomp2graph.hip)
template <class SRC>
static int c2g_build(mf_ctx *ctx, SRC &src, const uint32_t *val, uint64_t n_comps, int k, mf_gfa *out) {
    typedef typename SRC::keys KEYS;
    hipStream_t st = ctx->stream;
    const uint64_t nr = src.n(), nn = 2 * nr;
    if (!nr) return MF_OK;
    if (n_comps >= 0xFFFFFFFFull) return mf_set_error("comp2graph: %llu components (fewer than 2^32 - 1 are supported)", (unsigned long long)n_comps);
    const uint32_t nc = (uint32_t)n_comps;
    const bool even = (k & 1) == 0;
    // U1 per row, as comp2seq
    MF_TRY(src.index(ctx, k));                               // (the pair index stays with src: the link look-ups below probe it again)
    mf_buf<uint8_t> info, pal; mf_buf<uint32_t> ridx, lidx, succ;
    MF_TRY(info.alloc(ctx, nr)); MF_TRY(ridx.alloc(ctx, nr)); MF_TRY(lidx.alloc(ctx, nr)); MF_TRY(succ.alloc(ctx, nn));
    if (even) MF_TRY(pal.alloc(ctx, nr));
    ut_arrays A{};
    A.n = nr; A.k = k; A.info = info.p; A.ridx = ridx.p; A.lidx = lidx.p; A.pal = even ? pal.p : nullptr;
    MF_TRY(src.flags(ctx, A));
    const KEYS K = src.get();
    {
        mf_ktimer tm(ctx, "k_c2g_links");
        k_c2g_links<<<c2s_grid(nr), 256, 0, st>>>(info.p, ridx.p, lidx.p, A.pal, nr, succ.p);
    }
    info.reset(); ridx.reset(); lidx.reset();
    // heads, distances, cycle labels
    mf_buf<uint64_t> w0, w1; mf_buf<uint32_t> m0, m1; mf_buf<unsigned int> ctr;
    MF_TRY(w0.alloc(ctx, nn)); MF_TRY(w1.alloc(ctx, nn)); MF_TRY(m0.alloc(ctx, nn)); MF_TRY(m1.alloc(ctx, nn)); MF_TRY(ctr.alloc(ctx, 4));
    {
        mf_ktimer tm(ctx, "k_c2g_double");
        k_c2g_init<<<c2s_grid(nn), 256, 0, st>>>(succ.p, nn, w0.p, m0.p);
    }
    uint64_t prev = ~0ull;
    for (int round = 1; round <= 33; round++) {
        unsigned int open = 0;
        MF_HIP(hipMemsetAsync(ctr.p, 0, 4, st));
        {
            mf_ktimer tm(ctx, "k_c2g_double");
            k_c2g_double<<<c2s_grid(nn), 256, 0, st>>>(w0.p, m0.p, nn, w1.p, m1.p, ctr.p);
        }
        MF_HIP(hipMemcpyAsync(&open, ctr.p, 4, hipMemcpyDeviceToHost, st));
        MF_HIP(hipStreamSynchronize(st));
        w0.swap(w1); m0.swap(m1);
        // the open nodes of a path at least halve every round; what stays open are the nodes of cycles, and a round r label has seen
        // 2^r predecessors: done when that covers the longest cycle there can be
        if (open == 0 || ((uint64_t)open == prev && (round >= 32 || (1ull << round) >= (uint64_t)open))) break;
        prev = open;
    }
    w1.reset(); m1.reset();
    c2g_graph G{src.comp(), A.pal, succ.p, w0.p, m0.p, nr, k};
    // which strand, which cycles; segment ids
    mf_buf<uint32_t> plen, clen, off; mf_buf<uint64_t> P, Cy, tot;
    MF_TRY(plen.alloc(ctx, nn)); MF_TRY(clen.alloc(ctx, nn)); MF_TRY(off.alloc(ctx, (uint64_t)nc + 2)); MF_TRY(P.alloc(ctx, nn + 1)); MF_TRY(Cy.alloc(ctx, nn + 1));
    MF_TRY(tot.alloc(ctx, 4));
    MF_HIP(hipMemsetAsync(plen.p, 0, nn * 4, st)); MF_HIP(hipMemsetAsync(clen.p, 0, nn * 4, st)); MF_HIP(hipMemsetAsync(ctr.p, 0, 16, st));
    uint64_t n_paths = 0, n_cyc = 0;
    {
        mf_ktimer tm(ctx, "k_c2g_ends");
        k_c2g_ends<<<c2s_grid(nn), 256, 0, st>>>(G, plen.p, clen.p, ctr.p + 1);
        k_c2g_comp_off<<<c2s_grid(nr), 256, 0, st>>>(src.comp(), nr, nc, off.p);
    }
    mf_buf<uint32_t> flagp, flagc;
    MF_TRY(flagp.alloc(ctx, nn)); MF_TRY(flagc.alloc(ctx, nn));
    {
        mf_ktimer tm(ctx, "k_c2g_assign");
        k_c2g_nonzero<<<c2s_grid(nn), 256, 0, st>>>(plen.p, clen.p, nn, flagp.p, flagc.p);
        MF_TRY(mf_scan<1>(ctx, flagp.p, P.p, nn, tot.p));
        MF_TRY(mf_scan<1>(ctx, flagc.p, Cy.p, nn, tot.p + 1));
    }
    MF_HIP(hipMemcpyAsync(&n_paths, tot.p, 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipMemcpyAsync(&n_cyc, tot.p + 1, 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    flagp.reset(); flagc.reset();
    const uint64_t ns = n_paths + n_cyc;
    if (ns >= 0x7FFFFFFFull) return mf_set_error("comp2graph: %llu segments (fewer than 2^31 - 1 are supported)", (unsigned long long)ns);
    mf_buf<uint32_t> rseg, rpos, sstart, slen, scomp; mf_buf<uint8_t> ror; mf_buf<uint64_t> segbase;
    MF_TRY(rseg.alloc(ctx, nr)); MF_TRY(rpos.alloc(ctx, nr)); MF_TRY(ror.alloc(ctx, nr)); MF_TRY(sstart.alloc(ctx, ns)); MF_TRY(slen.alloc(ctx, ns));
    MF_TRY(scomp.alloc(ctx, ns)); MF_TRY(segbase.alloc(ctx, (uint64_t)nc + 1));
    c2g_segs S{rseg.p, rpos.p, ror.p, sstart.p, slen.p, scomp.p};
    MF_HIP(hipMemsetAsync(rseg.p, 0xFF, nr * 4, st));        // C2G_NONE: no segment yet
    MF_HIP(hipMemsetAsync(slen.p, 0, (ns ? ns : 1) * 4, st));
    {
        mf_ktimer tm(ctx, "k_c2g_assign");
        k_c2g_assign<<<c2s_grid(nn), 256, 0, st>>>(G, plen.p, clen.p, P.p, Cy.p, off.p, S);
        k_c2g_comp_base<<<c2s_grid((uint64_t)nc + 1), 256, 0, st>>>(P.p, Cy.p, off.p, nc, segbase.p);
    }
    MF_HIP(hipStreamSynchronize(st));
    plen.reset(); clen.reset(); P.reset(); Cy.reset(); w0.reset(); m0.reset(); succ.reset();
    G.succ = nullptr; G.word = nullptr; G.mn = nullptr;
    // rows in segment order; KC, printed strand, S line lengths
    mf_buf<uint64_t> soff, vsum, kc, es; mf_buf<uint32_t> nodeat, valat, sline; mf_buf<uint8_t> cmp;
    MF_TRY(soff.alloc(ctx, ns + 1)); MF_TRY(vsum.alloc(ctx, nr + 1)); MF_TRY(kc.alloc(ctx, ns)); MF_TRY(es.alloc(ctx, ns + 1));
    MF_TRY(nodeat.alloc(ctx, nr)); MF_TRY(valat.alloc(ctx, nr)); MF_TRY(sline.alloc(ctx, ns)); MF_TRY(cmp.alloc(ctx, ns));
    c2g_lines L{cmp.p, kc.p, sline.p};
    {
        mf_ktimer tm(ctx, "k_c2g_segments");
        MF_TRY(mf_scan<1>(ctx, slen.p, soff.p, ns, tot.p));
    }
    uint64_t covered = 0;
    unsigned int placed = 0;
    MF_HIP(hipMemcpyAsync(&covered, tot.p, 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    if (covered != nr) return mf_set_error("comp2graph: internal error, the segments hold %llu of %llu k-mers", (unsigned long long)covered, (unsigned long long)nr);
    {
        mf_ktimer tm(ctx, "k_c2g_segments");
        k_c2g_place<<<c2s_grid(nr), 256, 0, st>>>(S, soff.p, val, nr, ns, nodeat.p, valat.p, ctr.p);
    }
    MF_HIP(hipMemcpyAsync(&placed, ctr.p, 4, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    if (placed & 8u) return mf_set_error("comp2graph: internal error, a k-mer belongs to no segment");
    {
        mf_ktimer tm(ctx, "k_c2g_segments");
        MF_TRY(mf_scan<1>(ctx, valat.p, vsum.p, nr, tot.p + 1));
        k_c2g_segments<KEYS><<<c2s_grid(ns), 256, 0, st>>>(K, G, S, ns, soff.p, nodeat.p, valat.p, vsum.p, segbase.p, L);
        MF_TRY(mf_scan<1>(ctx, sline.p, es.p, ns, tot.p + 2));
    }
    // links
    mf_buf<uint32_t> lcnt, llen; mf_buf<uint16_t> zero, zero2; mf_buf<uint64_t> loff, rec, recs, el, lbase, seqoff;
    MF_TRY(lcnt.alloc(ctx, 2 * ns)); MF_TRY(loff.alloc(ctx, 2 * ns + 1));
    uint64_t nl = 0;
    {
        mf_ktimer tm(ctx, "k_c2g_links_of");
        k_c2g_links_of<0, KEYS><<<c2s_grid(2 * ns), 256, 0, st>>>(K, G, S, ns, soff.p, nodeat.p, cmp.p, lcnt.p, nullptr, nullptr, ctr.p);
        MF_TRY(mf_scan<1>(ctx, lcnt.p, loff.p, 2 * ns, tot.p + 3));
    }
    MF_HIP(hipMemcpyAsync(&nl, tot.p + 3, 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    MF_TRY(rec.alloc(ctx, nl)); MF_TRY(recs.alloc(ctx, nl)); MF_TRY(zero.alloc(ctx, nl)); MF_TRY(zero2.alloc(ctx, nl)); MF_TRY(llen.alloc(ctx, nl));
    MF_TRY(el.alloc(ctx, nl + 1)); MF_TRY(lbase.alloc(ctx, (uint64_t)nc + 1)); MF_TRY(seqoff.alloc(ctx, ns));
    if (nl) {
        MF_HIP(hipMemsetAsync(zero.p, 0, nl * 2, st));      // (mf_sort.hip has no keys-only sort: the narrowest value it carries)
        {
            mf_ktimer tm(ctx, "k_c2g_links_of");
            k_c2g_links_of<1, KEYS><<<c2s_grid(2 * ns), 256, 0, st>>>(K, G, S, ns, soff.p, nodeat.p, cmp.p, nullptr, loff.p, rec.p, ctr.p);
        }
        int bits = 34; while (bits < 64 && (1ull << (bits - 33)) < ns) bits++;
        MF_TRY(mf_sort_pairs(ctx, rec.p, zero.p, nl, bits, recs.p, zero2.p));
    }
    {
        mf_ktimer tm(ctx, "k_c2g_link_len");
        if (nl) k_c2g_link_len<<<c2s_grid(nl), 256, 0, st>>>(recs.p, nl, scomp.p, segbase.p, k, llen.p);
        MF_TRY(mf_scan<1>(ctx, llen.p, el.p, nl, tot.p + 3));
        k_c2g_link_base<<<c2s_grid((uint64_t)nc + 1), 256, 0, st>>>(recs.p, nl, segbase.p, nc, lbase.p);
    }
    uint64_t tb[4] = {0, 0, 0, 0}; unsigned int fl[4] = {0, 0, 0, 0};
    MF_HIP(hipMemcpyAsync(tb, tot.p, 32, hipMemcpyDeviceToHost, st));
    MF_HIP(hipMemcpyAsync(fl, ctr.p, 16, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    if (fl[0] & 4u) return mf_set_error("comp2graph: internal error, a link ends inside a segment");
    const uint64_t bytes = tb[2] + tb[3];
    void *text = nullptr;
    MF_TRY(mf_alloc(ctx, bytes ? bytes : 1, &text));
    out->d_text = (uint8_t *)text; out->text_bytes = bytes ? bytes : 1;
    c2g_text T{es.p, el.p, segbase.p, lbase.p, seqoff.p, out->d_text};
    {
        mf_ktimer tm(ctx, "k_c2g_write");
        k_c2g_write_s<<<c2s_grid(ns), 256, 0, st>>>(S, ns, L, T, k);
        k_c2g_write_bases<KEYS><<<c2s_grid(nr), 256, 0, st>>>(K, G, S, L, T);
        if (nl) k_c2g_write_l<<<c2s_grid(nl), 256, 0, st>>>(recs.p, nl, scomp.p, T, k);
    }
    MF_HIP(hipStreamSynchronize(st));
    MF_HIP(hipGetLastError());
    out->n_bytes = bytes; out->n_segments = ns; out->n_links = nl; out->n_cycles = n_cyc;
    return MF_OK;
}

// the host only writes the buffer
static int c2g_write_text(mf_ctx *ctx, const mf_gfa &g, const char *out_gfa) {
    FILE *f = fopen(out_gfa, "w");
    if (!f) return mf_set_error("can't write '%s'", out_gfa);
    bool bad = false;
    const uint64_t piece = 64ull << 20;
    std::vector<uint8_t> buf((size_t)std::min<uint64_t>(piece, std::max<uint64_t>(g.n_bytes, 1)));
    for (uint64_t at = 0; at < g.n_bytes && !bad; at += piece) {
        const uint64_t m = std::min<uint64_t>(piece, g.n_bytes - at);
        if (hipMemcpyAsync(buf.data(), g.d_text + at, m, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) { bad = true; break; }
        bad = fwrite(buf.data(), 1, m, f) != m;
    }
    if (fclose(f) != 0 || bad) return mf_set_error("can't write '%s'", out_gfa);
    return MF_OK;
}
// the text of a mf_gfa on the stack goes back to the arena with it
struct c2g_text_guard { mf_gfa &g; ~c2g_text_guard() { if (g.d_text) mf_release(g.ctx, g.d_text, g.text_bytes); } };
