// Host-side planners of the grouped weight-gradient kernels (wgrad_group.hip: bf16, wgrad_f32.hip: f32): they cut a list of
// products dW_p += dY_p^T X_p into the work items the kernels walk.  Plain C++17, no HIP: the two entry points include this header,
// and so does tests/host/wgrad_plan_check.cpp, which checks the plans' invariants without a GPU (every tile's reduction covered
// exactly once, cut tiles atomic, every item reached by the kernels' walk).  Item and ItemF are also the device-side records.
#ifndef S2T_WGRAD_PLAN_HPP
#define S2T_WGRAD_PLAN_HPP
#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

namespace wgrad_plan {
// ================================================================== bf16: wgrad_group.hip
constexpr int TILE = 256, KTILE = 64;      // output tile (rows and columns), tokens per K-tile (BK of gemm_tile.hpp)
// one work item = one 256 x 256 output tile over the K-tiles [kt0, kt1) of its problem.  `atomic`: the tile's token range is
// shared with other items (a tile that straddles two workgroups' shares), so the result is ADDED with f32 atomics.
struct Item { int prob, tm, tn, kt0, kt1, atomic; };

// ---- work lists.  A list is a table [round][slot]: workgroup slot s runs items s, s + G, s + 2G, ... until an empty one.
// Cost model for comparing lists: an item costs its K-tiles plus C0 (pipeline fill from cold operands + the epilogue's 256 KB
// read-modify-write, measured ~8 K-tile times at 40-K-tile items); a launch takes as long as its most loaded slot.
constexpr int C0 = 8, MINP = 8;
struct Layout { std::vector<Item> table; int used = 0; long makespan = 0; bool fill = false; };

inline long load_of(const Layout& L) {
    long worst = 0;
    for (int sl = 0; sl < L.used; ++sl) {
        long u = 0;
        for (size_t it = sl; it < L.table.size(); it += L.used) {
            const Item& t = L.table[it];
            if (t.kt0 >= t.kt1) break;
            u += t.kt1 - t.kt0 + C0;
        }
        worst = std::max(worst, u);
    }
    return worst;
}

// the whole-reduction tiles of problem `prob`, row-major over (tm, tn), appended to iv
inline void push_tiles(std::vector<Item>& iv, int prob, int n_out, int n_in, int tokens) {
    const int nk = (tokens + KTILE - 1) / KTILE, tn = (n_in + TILE - 1) / TILE, tmn = (n_out + TILE - 1) / TILE;
    for (int a = 0; a < tmn; ++a)
        for (int b = 0; b < tn; ++b) iv.push_back(Item{prob, a, b, 0, nk, 0});
}

// Layout 1 -- rounds.  Longest reductions first (stable: the tiles of one dW stay neighbours), dealt in rounds of one item per CU; the
// workgroups of a round sweep the token range of neighbouring tiles in step, which is what lets the L2s / the MALL serve the
// operand columns those tiles share (a schedule that balanced the CUs perfectly by handing each an arbitrary stretch of a line
// of tiles ran 1.6x SLOWER: every tile then streams its 24 MB of operands from HBM alone).  Two cuts along the token range, whose
// pieces meet in f32 atomics:
//  * a tile whose reduction is much longer than a CU's fair share of the launch is cut into equal pieces of about that share, the
//    same token ranges for all tiles of its dW;
//  * a partly filled last round would leave CUs idle for a whole item's time: its items are cut into as many equal pieces as
//    fill the round.
// The right list for uniform groups (the encoder's 616 tiles of 375 K-tiles).  G: workgroups of the launch.
inline void layout_rounds(std::vector<Item> iv, int G, Layout& out) {
    long units = 0;
    for (const Item& t : iv) units += t.kt1 + 6;
    const int share = (int)((units + G - 1) / G);
    {
        std::vector<Item> cutv;
        cutv.reserve(iv.size());
        for (size_t i = 0; i < iv.size();) {
            size_t j = i;
            while (j < iv.size() && iv[j].prob == iv[i].prob) ++j;           // the tiles of one dW: same reduction length
            const int nk = iv[i].kt1;
            const int f = nk > share + share / 4 ? std::min((nk + share - 1) / share, nk / MINP) : 1;
            if (f <= 1) cutv.insert(cutv.end(), iv.begin() + i, iv.begin() + j);
            else {
                const int per = (nk + f - 1) / f;
                for (int piece = 0; piece < f; ++piece)                      // piece-major: equal token ranges sit next to each other
                    for (size_t k = i; k < j; ++k) {
                        const int k0 = piece * per, k1 = std::min(nk, k0 + per);
                        if (k0 < k1) cutv.push_back(Item{iv[k].prob, iv[k].tm, iv[k].tn, k0, k1, 1});
                    }
            }
            i = j;
        }
        iv.swap(cutv);
    }
    std::stable_sort(iv.begin(), iv.end(), [](const Item& x, const Item& y) { return x.kt1 - x.kt0 > y.kt1 - y.kt0; });
    const int rem = (int)(iv.size() % G);
    if (rem) {
        const int f = G / rem;
        if (f >= 2) {
            std::vector<Item> tail(iv.end() - rem, iv.end());
            iv.resize(iv.size() - rem);
            for (int piece = 0; piece < f; ++piece)
                for (const Item& t : tail) {
                    const int nk = t.kt1 - t.kt0, ff = std::max(1, std::min(f, nk / MINP)), per = (nk + ff - 1) / ff;
                    const int k0 = t.kt0 + piece * per, k1 = std::min(t.kt1, k0 + per);
                    if (piece < ff && k0 < k1) iv.push_back(Item{t.prob, t.tm, t.tn, k0, k1, ff > 1 ? 1 : t.atomic});
                }
        }
    }
    out.used = (int)std::min<size_t>(iv.size(), G);
    out.table.swap(iv);
    out.fill = false;
    out.makespan = load_of(out);
}

// Layout 2 -- fill to a level.  For groups that mix a few very long reductions with many short ones (the decoder's: six K/V
// projections over the ~24,000 source tokens = 48 tiles of 374 K-tiles next to 400 tiles of 40 K-tiles over its own 2,560 tokens):
// the short tiles are dealt over the slots whole (1 or 2 each), then the long dWs are poured into what is left of every slot up to
// a common level T: the tiles of one dW always as a gang on neighbouring slots with the SAME token range (they sweep it in step, first
// thing in their slots), the range cut wherever a gang's slots are full.  Every slot ends within a few K-tiles of T.
inline bool layout_fill(const std::vector<Item>& tiles, int G, Layout& out) {
    struct Line { size_t first, count; int nk; };
    std::vector<Line> lines;
    long units = 0;
    for (size_t i = 0; i < tiles.size();) {
        size_t j = i;
        while (j < tiles.size() && tiles[j].prob == tiles[i].prob) ++j;
        lines.push_back(Line{i, j - i, tiles[i].kt1});
        units += (long)(j - i) * (tiles[i].kt1 + C0);
        i = j;
    }
    const long fair = units / G;
    std::vector<Line> longs;
    std::vector<Item> shorts;
    long long_k = 0;
    for (const Line& l : lines) {
        if (l.nk + C0 > fair && l.count <= (size_t)G / 2 && l.nk >= 4 * MINP) { longs.push_back(l); long_k += (long)l.count * l.nk; }
        else shorts.insert(shorts.end(), tiles.begin() + l.first, tiles.begin() + l.first + l.count);
    }
    if (longs.empty()) return false;
    std::stable_sort(shorts.begin(), shorts.end(), [](const Item& x, const Item& y) { return x.kt1 > y.kt1; });
    std::vector<std::vector<Item>> tail(G), head(G);
    std::vector<long> base(G, 0);
    for (size_t i = 0; i < shorts.size(); ++i) { tail[i % G].push_back(shorts[i]); base[i % G] += shorts[i].kt1 + C0; }
    long sum_base = 0;
    for (long b : base) sum_base += b;
    std::vector<long> ld;
    long T = (sum_base + long_k + (long)G * C0 + G - 1) / G;
    for (int attempt = 0; attempt < 64; ++attempt, T += std::max(1L, T / 64)) {
        for (auto& h : head) h.clear();
        ld = base;
        size_t sl = 0;
        bool ok = true;
        for (const Line& l : longs) {
            int k0 = 0;
            while (k0 < l.nk && ok) {
                if (sl + l.count > (size_t)G) { ok = false; break; }
                long cap = T;
                for (size_t j = 0; j < l.count; ++j) cap = std::min(cap, T - ld[sl + j] - C0);
                int len = (int)std::min<long>(cap, l.nk - k0);
                if (l.nk - k0 - len > 0 && l.nk - k0 - len < MINP) len = l.nk - k0 - MINP;     // never leave a remainder shorter than MINP
                if (len < MINP) { sl += l.count; continue; }                                    // this gang is full
                for (size_t j = 0; j < l.count; ++j) {
                    const Item& t = tiles[l.first + j];
                    head[sl + j].push_back(Item{t.prob, t.tm, t.tn, k0, k0 + len, len == l.nk ? 0 : 1});
                    ld[sl + j] += len + C0;
                }
                k0 += len;
            }
            if (!ok) break;
        }
        if (!ok) continue;
        size_t rounds = 0;
        for (int i = 0; i < G; ++i) rounds = std::max(rounds, head[i].size() + tail[i].size());
        out.table.assign(rounds * G, Item{0, 0, 0, 0, 0, 0});
        for (int i = 0; i < G; ++i) {
            size_t r = 0;
            for (const Item& t : head[i]) out.table[(r++) * G + i] = t;
            for (const Item& t : tail[i]) out.table[(r++) * G + i] = t;
        }
        out.used = G;
        out.fill = true;
        out.makespan = load_of(out);
        return true;
    }
    return false;
}

// the list the kernel runs: the fill layout where it exists and its most loaded slot is lighter than the rounds layout's
inline Layout plan(std::vector<Item> iv, int G) {
    Layout lay, alt;
    const bool have_alt = layout_fill(iv, G, alt);
    layout_rounds(std::move(iv), G, lay);
    if (have_alt && alt.makespan < lay.makespan) std::swap(lay, alt);
    return lay;
}

// ================================================================== f32: wgrad_f32.hip
constexpr int TILE_F32 = 128, STAGE_F32 = 32, SLOTS_F32 = 512;     // output tile, tokens per stage, workgroups of a full launch
struct ItemF { int prob, tm, tn, s0, s1, atomic; };              // stages [s0, s1) of 32 tokens; atomic: a piece of a tile cut along the tokens

inline void push_tiles_f32(std::vector<ItemF>& iv, int prob, int n_out, int n_in, int tokens) {
    for (int a = 0; a < (n_out + TILE_F32 - 1) / TILE_F32; ++a)
        for (int b = 0; b < (n_in + TILE_F32 - 1) / TILE_F32; ++b) iv.push_back(ItemF{prob, a, b, 0, (tokens + STAGE_F32 - 1) / STAGE_F32, 0});
}

// longest reductions first, dealt round-robin to the workgroups (workgroup b runs items b, b + grid, ...): a launch takes as long
// as its most loaded workgroup
inline void plan_f32(std::vector<ItemF>& iv) {
    constexpr int SLOTS = SLOTS_F32;
    auto len = [](const ItemF& t) { return t.s1 - t.s0; };
    std::stable_sort(iv.begin(), iv.end(), [&](const ItemF& x, const ItemF& y) { return len(x) > len(y); });
    {   // the long class = items at least half as long as the longest; its partly filled last round is cut to fill the round
        size_t L = 0;
        while (L < iv.size() && 2 * len(iv[L]) >= len(iv[0])) ++L;
        const size_t rem = L % SLOTS;
        if (L > SLOTS && rem > 0 && rem <= SLOTS / 2 && len(iv[0]) >= 16) {
            const int f = (int)std::min<size_t>(8, SLOTS / rem);
            std::vector<ItemF> cut;
            for (size_t i = L - rem; i < L; ++i) {
                const int n = len(iv[i]), per = (n + f - 1) / f;
                for (int c = 0; c < n; c += per) cut.push_back(ItemF{iv[i].prob, iv[i].tm, iv[i].tn, c, std::min(n, c + per), 1});
            }
            iv.erase(iv.begin() + (L - rem), iv.begin() + L);
            iv.insert(iv.end(), cut.begin(), cut.end());
            std::stable_sort(iv.begin(), iv.end(), [&](const ItemF& x, const ItemF& y) { return len(x) > len(y); });
        }
    }
}
inline int grid_f32(size_t n_items) { return (int)std::min<size_t>(n_items, SLOTS_F32); }
}  // namespace wgrad_plan
#endif
