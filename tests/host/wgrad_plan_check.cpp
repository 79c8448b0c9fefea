// Host check of the work-list planners of the grouped weight-gradient kernels (fbk_fairseq_st_amd/csrc/wgrad_plan.hpp), no GPU:
//   wgrad_plan_check random N SEED     N seeded random lists through EACH planner, every invariant below on each list
//   wgrad_plan_check edges             the smallest list, the longest list (4,096 products), one product far above the fair share
//   wgrad_plan_check plan bf16|f32 G   a list read from stdin (lines "count n_out n_in tokens"): invariants, then one line of facts
// Invariants (a violation prints the list's shape and ends the program with status 1):
//   every (problem, tm, tn) tile appears; its pieces are disjoint and cover [0, nk) exactly; a tile of several pieces is atomic on
//   all of them; item fields are in range; 1 <= used <= G (bf16), grid = min(items, 512) (f32); walking slot s as the kernels do
//   (s, s + used, ..., stopping at the first empty item) reaches every non-empty item exactly once; the reported makespan is
//   load_of recomputed; the chosen bf16 layout is the one with the smaller makespan; the same input gives the same plan twice.
// tests/test_wgrad_plan_cpu.py builds and runs this.
#include "wgrad_plan.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

namespace wp = wgrad_plan;

namespace {
struct Shape { int n_out, n_in, tokens; };
struct Facts { long items = 0, cut_tiles = 0, atomic_items = 0, min_pieces = 0, max_pieces = 0, makespan = 0; int used = 0; bool fill = false; };

std::string g_what;                       // the list under test, for failure messages
[[noreturn]] void fail(const char* msg, long a = 0, long b = 0, long c = 0) {
    std::fprintf(stderr, "FAIL %s: %s (%ld, %ld, %ld)\n", g_what.c_str(), msg, a, b, c);
    std::exit(1);
}
#define CHECK(cond, ...) do { if (!(cond)) fail(#cond, ##__VA_ARGS__); } while (0)

int cdiv(int a, int b) { return (a + b - 1) / b; }

// pieces of every tile: disjoint, union exactly [0, nk), several pieces => atomic on all
template <typename It, typename Lo, typename Hi>
void check_cover(const std::vector<Shape>& shapes, const std::vector<It>& items, int tile, int ktile, Lo lo, Hi hi, Facts& f) {
    std::vector<long> first(shapes.size() + 1, 0);                               // tile index of (prob, 0, 0)
    for (size_t i = 0; i < shapes.size(); ++i) first[i + 1] = first[i] + (long)cdiv(shapes[i].n_out, tile) * cdiv(shapes[i].n_in, tile);
    struct Piece { long tile; int lo, hi, atomic; };
    std::vector<Piece> pieces;
    pieces.reserve(items.size());
    for (const It& t : items) {
        if (lo(t) >= hi(t)) continue;
        CHECK(t.prob >= 0 && t.prob < (int)shapes.size(), t.prob);
        const Shape& s = shapes[t.prob];
        CHECK(t.tm >= 0 && t.tm < cdiv(s.n_out, tile) && t.tn >= 0 && t.tn < cdiv(s.n_in, tile), t.prob, t.tm, t.tn);
        CHECK(lo(t) >= 0 && hi(t) <= cdiv(s.tokens, ktile), t.prob, lo(t), hi(t));
        CHECK(t.atomic == 0 || t.atomic == 1, t.atomic);
        pieces.push_back(Piece{first[t.prob] + (long)t.tm * cdiv(s.n_in, tile) + t.tn, lo(t), hi(t), t.atomic});
        ++f.items;
        f.atomic_items += t.atomic;
    }
    std::sort(pieces.begin(), pieces.end(), [](const Piece& x, const Piece& y) { return x.tile != y.tile ? x.tile < y.tile : x.lo < y.lo; });
    size_t i = 0;
    for (size_t p = 0; p < shapes.size(); ++p)
        for (long tl = first[p]; tl < first[p + 1]; ++tl) {
            CHECK(i < pieces.size() && pieces[i].tile == tl, (long)p, tl);       // every tile appears
            size_t j = i;
            int at = 0;
            for (; j < pieces.size() && pieces[j].tile == tl; ++j) {
                CHECK(pieces[j].lo == at, (long)p, at, pieces[j].lo);             // no gap, no overlap
                at = pieces[j].hi;
            }
            CHECK(at == cdiv(shapes[p].tokens, ktile), (long)p, at);              // the union is [0, nk)
            const long n = (long)(j - i);
            for (; i < j; ++i) CHECK(n == 1 || pieces[i].atomic == 1, (long)p, n);
            if (n > 1) {
                ++f.cut_tiles;
                f.min_pieces = f.min_pieces ? std::min(f.min_pieces, n) : n;
                f.max_pieces = std::max(f.max_pieces, n);
            }
        }
    CHECK(i == pieces.size(), (long)i, (long)pieces.size());
}

bool same(const wp::Layout& a, const wp::Layout& b) {
    return a.used == b.used && a.makespan == b.makespan && a.fill == b.fill && a.table.size() == b.table.size() &&
           (a.table.empty() || std::memcmp(a.table.data(), b.table.data(), a.table.size() * sizeof(wp::Item)) == 0);
}

void check_layout(const std::vector<Shape>& shapes, const wp::Layout& L, int G, Facts& f) {
    CHECK(L.used >= 1 && L.used <= G, L.used, G);
    std::vector<char> seen(L.table.size(), 0);
    for (int s = 0; s < L.used; ++s)                                              // the kernel's walk
        for (size_t it = s; it < L.table.size(); it += L.used) {
            if (L.table[it].kt0 >= L.table[it].kt1) break;
            CHECK(!seen[it], (long)it);
            seen[it] = 1;
        }
    for (size_t it = 0; it < L.table.size(); ++it)
        CHECK(seen[it] || L.table[it].kt0 >= L.table[it].kt1, (long)it, L.used, (long)L.table.size());   // an item no workgroup reaches
    check_cover(shapes, L.table, wp::TILE, wp::KTILE, [](const wp::Item& t) { return t.kt0; }, [](const wp::Item& t) { return t.kt1; }, f);
    CHECK(L.makespan == wp::load_of(L), L.makespan, wp::load_of(L));
}

Facts check_bf16(const std::vector<Shape>& shapes, int G) {
    std::vector<wp::Item> iv;
    for (size_t i = 0; i < shapes.size(); ++i) wp::push_tiles(iv, (int)i, shapes[i].n_out, shapes[i].n_in, shapes[i].tokens);
    const wp::Layout L = wp::plan(iv, G);
    Facts f;
    check_layout(shapes, L, G, f);
    // both candidates are valid plans, and the chosen one is the lighter (rounds on a tie)
    wp::Layout r, a;
    wp::layout_rounds(iv, G, r);
    Facts fr, fa;
    check_layout(shapes, r, G, fr);
    const bool have = wp::layout_fill(iv, G, a);
    if (have) check_layout(shapes, a, G, fa);
    CHECK(L.fill == (have && a.makespan < r.makespan), L.fill, have ? a.makespan : -1, r.makespan);
    CHECK(L.makespan == (have ? std::min(a.makespan, r.makespan) : r.makespan), L.makespan);
    CHECK(same(L, L.fill ? a : r));
    CHECK(same(L, wp::plan(iv, G)));                                              // the same input, the same plan
    f.used = L.used; f.makespan = L.makespan; f.fill = L.fill;
    return f;
}

Facts check_f32(const std::vector<Shape>& shapes) {
    std::vector<wp::ItemF> iv;
    for (size_t i = 0; i < shapes.size(); ++i) wp::push_tiles_f32(iv, (int)i, shapes[i].n_out, shapes[i].n_in, shapes[i].tokens);
    std::vector<wp::ItemF> again = iv;
    wp::plan_f32(iv);
    wp::plan_f32(again);
    CHECK(iv.size() == again.size() && std::memcmp(iv.data(), again.data(), iv.size() * sizeof(wp::ItemF)) == 0);
    const int grid = wp::grid_f32(iv.size());
    CHECK(grid == (int)std::min<size_t>(iv.size(), 512) && grid >= 1, grid);
    std::vector<char> seen(iv.size(), 0);
    for (int b = 0; b < grid; ++b)
        for (size_t it = b; it < iv.size(); it += grid) { CHECK(!seen[it], (long)it); seen[it] = 1; }
    for (size_t it = 0; it < iv.size(); ++it) CHECK(seen[it] && iv[it].s0 < iv[it].s1, (long)it);      // the kernel has no empty items
    Facts f;
    check_cover(shapes, iv, wp::TILE_F32, wp::STAGE_F32, [](const wp::ItemF& t) { return t.s0; }, [](const wp::ItemF& t) { return t.s1; }, f);
    CHECK(f.max_pieces <= 8, f.max_pieces);
    f.used = grid;
    return f;
}

// ---- seeded lists (splitmix64: the same lists with every compiler and library)
struct Rng {
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    int in(int lo, int hi) { return lo + (int)(next() % (uint64_t)(hi - lo + 1)); }                     // inclusive
    // small values as likely as large ones (the interesting plans mix tiny and huge): uniform in [lo, min(hi, lo * 2^k)], k random
    int skew(int lo, int hi) { int top = lo; const int k = in(0, 15); for (int i = 0; i < k && top < hi; ++i) top = std::min(hi, 2 * top + 1); return in(lo, top); }
};

std::string describe(const std::vector<Shape>& shapes, int G, const char* kind) {
    char buf[160];
    std::snprintf(buf, sizeof buf, "%s G=%d n=%zu first=(%d,%d,%d) last=(%d,%d,%d)", kind, G, shapes.size(), shapes[0].n_out, shapes[0].n_in,
                  shapes[0].tokens, shapes.back().n_out, shapes.back().n_in, shapes.back().tokens);
    return buf;
}

int run_random(long n_lists, uint64_t seed) {
    // workgroups of the bf16 launch: 256 - reserve_cus with reserve_cus in [0, 128] (s2t_set_option)
    const int Gs[] = {256, 255, 240, 200, 156};
    long fill = 0, cut = 0, cut_f32 = 0;
    for (long l = 0; l < 2 * n_lists; ++l) {                                     // even: bf16, odd: f32; n_lists of each
        Rng r{seed * 1000003ull + (uint64_t)l};
        const bool f32 = l & 1;
        const int lo = f32 ? 1 : 8;
        const int n = (l / 2) % 10 == 9 ? r.in(1, 700) : r.in(1, 30);
        int cls[3];
        const int ncls = r.in(1, 3);
        for (int c = 0; c < ncls; ++c) cls[c] = r.in(0, 1) ? r.in(1, 30000) : r.skew(1, 30000);
        const bool small = r.in(0, 1);                                            // half the lists: mostly tiny products (tiles counted, not sized)
        std::vector<Shape> shapes(n);
        for (Shape& s : shapes) {
            s.n_out = small ? r.skew(lo, 2200) : r.in(lo, 2200);
            s.n_in = small ? r.skew(lo, 2200) : r.in(lo, 2200);
            s.tokens = cls[r.in(0, ncls - 1)];
        }
        const int G = Gs[r.in(0, 4)];
        g_what = describe(shapes, G, f32 ? "random f32" : "random bf16") + " list " + std::to_string(l);
        if (f32) cut_f32 += check_f32(shapes).cut_tiles > 0;
        else { const Facts f = check_bf16(shapes, G); fill += f.fill; cut += f.cut_tiles > 0; }
    }
    std::printf("ok random lists_bf16=%ld lists_f32=%ld fill=%ld cut=%ld cut_f32=%ld\n", n_lists, n_lists, fill, cut, cut_f32);
    return 0;
}

int run_edges() {
    const int Gs[] = {256, 255, 240, 200, 156};
    for (int G : Gs) {
        std::vector<std::vector<Shape>> lists;
        lists.push_back({Shape{8, 8, 1}});
        lists.push_back(std::vector<Shape>(4096, Shape{8, 8, 1}));                // WGRAD_GROUP_MAX products
        lists.push_back(std::vector<Shape>(4096, Shape{300, 8, 2048}));
        lists.push_back({Shape{256, 256, 30000}});                                // nk far above the fair share, alone
        lists.push_back({Shape{2200, 2200, 30000}});
        lists.push_back({Shape{256, 256, 30000}, Shape{8, 8, 1}});
        for (const auto& s : lists) {
            g_what = describe(s, G, "edge bf16");
            const Facts f = check_bf16(s, G);
            if (s.size() == 1 && s[0].tokens == 1) CHECK(f.items == 1 && f.used == 1 && f.atomic_items == 0, f.items, f.used);
            if (s.size() == 1 && s[0].n_out == 256 && s[0].tokens == 30000) CHECK(f.cut_tiles == 1 && f.max_pieces > 8, f.cut_tiles, f.max_pieces);
        }
    }
    std::vector<std::vector<Shape>> lists;
    lists.push_back({Shape{1, 1, 1}});
    lists.push_back(std::vector<Shape>(4096, Shape{1, 1, 1}));
    lists.push_back(std::vector<Shape>(4096, Shape{129, 1, 2048}));
    lists.push_back({Shape{128, 128, 30000}});
    lists.push_back({Shape{2200, 2200, 30000}});
    for (const auto& s : lists) {
        g_what = describe(s, 512, "edge f32");
        const Facts f = check_f32(s);
        if (s.size() == 1 && s[0].tokens == 1) CHECK(f.items == 1 && f.used == 1 && f.atomic_items == 0, f.items, f.used);
    }
    std::printf("ok edges\n");
    return 0;
}

int run_plan(const char* kind, int G) {
    std::vector<Shape> shapes;
    int count, n_out, n_in, tokens;
    while (std::scanf("%d %d %d %d", &count, &n_out, &n_in, &tokens) == 4)
        for (int i = 0; i < count; ++i) shapes.push_back(Shape{n_out, n_in, tokens});
    if (shapes.empty() || shapes.size() > 4096 || G < 1) { std::fprintf(stderr, "bad list\n"); return 2; }
    const bool f32 = !std::strcmp(kind, "f32");
    g_what = describe(shapes, G, kind);
    const Facts f = f32 ? check_f32(shapes) : check_bf16(shapes, G);
    std::printf("ok items=%ld cut_tiles=%ld atomic_items=%ld min_pieces=%ld max_pieces=%ld layout=%s makespan=%ld used=%d\n", f.items, f.cut_tiles,
                f.atomic_items, f.min_pieces, f.max_pieces, f32 ? "f32" : f.fill ? "fill" : "rounds", f.makespan, f.used);
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "random")) return run_random(std::atol(argv[2]), (uint64_t)std::atoll(argv[3]));
    if (argc == 2 && !std::strcmp(argv[1], "edges")) return run_edges();
    if (argc == 4 && !std::strcmp(argv[1], "plan")) return run_plan(argv[2], std::atoi(argv[3]));
    std::fprintf(stderr, "usage: %s random N SEED | edges | plan bf16|f32 G < list\n", argv[0]);
    return 2;
}
