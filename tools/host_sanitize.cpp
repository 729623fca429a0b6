// Sanitizer driver ("race / memory checking"): the host-only half of the C ABI (rls_host.cpp: the
// schedule builders every DeviceGraph and every MCPG visiting order go through) and the C oracle (oracle/oracle.c), run
// over random graphs -- G(n, m), stars and multi-hub graphs, paths, isolated nodes, N = 1, duplicate edges -- in
// EXACTLY-sized heap buffers, built with -fsanitize=address,undefined by tests/test_sanitize.py.  Every builder runs
// its sizing call first and then fills buffers of exactly that size, so a one-past-the-end write is an ASAN report;
// structural invariants (every node scheduled once, levels respect the dependency order, ELL rows complete) are checked
// on top.  The launch planners (csrc/rls_maxcut_plan.h, rls_ls_plan.h, rls_tsp_plan.h, rls_isco_plan.h, rls_subset_plan.h: host-only C++) run over random shapes beside them.  Exit code 0 = clean.  CPU only: sanitizers do not run on the GPU box.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "rlsolver_hip.h"
#include "rls_maxcut_plan.h"      // the MaxCut launch planner: host-only C++, so it runs under the sanitizers too
#include "rls_ls_plan.h"          // ... and the local search's
#include "rls_tsp_plan.h"         // ... and the TSP one
#include "rls_isco_plan.h"        // ... and the ISCO steps'
#include "rls_subset_plan.h"      // ... and sub_set_sampling's

#include "../oracle/oracle.h"

#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "host_sanitize: CHECK failed: %s | ", #cond); \
            std::fprintf(stderr, __VA_ARGS__);                             \
            std::fprintf(stderr, "\n");                                    \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

struct Graph {
    int64_t n;
    std::vector<int32_t> eu, ev;              // stored edges, sorted by (eu, ev)
    std::vector<int32_t> erowptr;             // [n + 1]
    std::vector<int32_t> rowptr, col;         // symmetric CSR, rows sorted
    int32_t max_deg;
};

static Graph make_graph(std::mt19937_64& rng, int kind) {
    auto U = [&](int64_t lo, int64_t hi) { return (int64_t)(lo + rng() % (uint64_t)(hi - lo + 1)); };
    Graph g;
    std::set<std::pair<int32_t, int32_t>> e;
    switch (kind) {
        case 0: g.n = 1; break;                                                        // N = 1, no edges
        case 1: g.n = U(2, 70); break;                                                 // tiny
        case 2: g.n = U(64, 700); break;
        case 3: g.n = U(700, 5000); break;
        default: g.n = U(100, 3000); break;
    }
    const int64_t n = g.n;
    auto add = [&](int64_t a, int64_t b) { if (a != b) e.insert({(int32_t)std::min(a, b), (int32_t)std::max(a, b)}); };
    if (n > 1) {
        if (kind == 4) {                                                               // hubs (degree up to 4000) + isolated nodes
            const int hubs = (int)U(1, 5);
            for (int h = 0; h < hubs; ++h) {
                const int64_t hub = U(0, n - 1), d = std::min<int64_t>(n - 1, U(60, 4000));
                for (int64_t k = 0; k < d; ++k) add(hub, U(0, n - 1));
            }
            for (int64_t k = U(0, n); k > 0; --k) add(U(0, n / 2), U(0, n / 2));        // the upper half stays mostly isolated
        } else if (kind == 5) {                                                        // path + chords
            for (int64_t i = 0; i + 1 < n; ++i) add(i, i + 1);
            for (int64_t i = 0; i + 2 < n; i += U(1, 5)) add(i, i + 2);
        } else {
            const int64_t m = U(kind == 1 ? 0 : 1, std::min<int64_t>(n * (n - 1) / 2, n * U(1, 12)));
            for (int64_t k = 0; k < m; ++k) add(U(0, n - 1), U(0, n - 1));
        }
    }
    for (auto& p : e) { g.eu.push_back(p.first); g.ev.push_back(p.second); }
    g.erowptr.assign((size_t)n + 1, 0);
    for (int32_t u : g.eu) ++g.erowptr[(size_t)u + 1];
    for (int64_t i = 0; i < n; ++i) g.erowptr[(size_t)i + 1] += g.erowptr[(size_t)i];
    std::vector<std::vector<int32_t>> adj((size_t)n);
    for (size_t k = 0; k < g.eu.size(); ++k) { adj[(size_t)g.eu[k]].push_back(g.ev[k]); adj[(size_t)g.ev[k]].push_back(g.eu[k]); }
    g.rowptr.assign((size_t)n + 1, 0);
    g.max_deg = 0;
    for (int64_t i = 0; i < n; ++i) {
        std::sort(adj[(size_t)i].begin(), adj[(size_t)i].end());
        g.rowptr[(size_t)i + 1] = g.rowptr[(size_t)i] + (int32_t)adj[(size_t)i].size();
        g.max_deg = std::max(g.max_deg, (int32_t)adj[(size_t)i].size());
        for (int32_t v : adj[(size_t)i]) g.col.push_back(v);
    }
    return g;
}

// exact-size heap array: reading or writing element [size] is an ASAN report
template <class T>
struct Exact {
    T* p;
    size_t n;
    explicit Exact(size_t n_) : p(new T[n_ ? n_ : 0]()), n(n_) {}
    ~Exact() { delete[] p; }
    T& operator[](size_t i) { return p[i]; }
};

static void run_builders(const Graph& g, std::mt19937_64& rng) {
    const int64_t N = g.n, nnz = (int64_t)g.col.size();
    const int32_t* rp = g.rowptr.data();
    const int32_t* col = g.col.empty() ? nullptr : g.col.data();
    // ---- rls_graph_sweep_schedule: every node once, followed by its row; a batch never mixes levels
    {
        Exact<int32_t> flagged((size_t)N + 1), stream((size_t)(nnz + N));
        int64_t nb = -1, nl = -1;
        CHECK(rls_graph_sweep_schedule(rp, col, N, 64, 768, flagged.p, stream.p, &nb, &nl) == RLS_OK, "%s", rls_last_error_string());
        std::vector<char> seen((size_t)N, 0);
        std::vector<int32_t> level((size_t)N, -1);
        int32_t cur = -1;
        for (int64_t k = 0; k < N; ++k) {
            const uint32_t f = (uint32_t)flagged[(size_t)k];
            const int64_t off = f & 0x7fffffffu;
            const int32_t node = stream[(size_t)off];
            CHECK(node >= 0 && node < N && !seen[(size_t)node], "node %d scheduled twice", node);
            seen[(size_t)node] = 1;
            if (f >> 31) ++cur;
            level[(size_t)node] = cur;
            const int64_t end = (uint32_t)flagged[(size_t)k + 1] & 0x7fffffffu;
            CHECK(end - off == 1 + rp[node + 1] - rp[node], "row length of node %d", node);
            for (int64_t j = 0; j < rp[node + 1] - rp[node]; ++j) CHECK(stream[(size_t)(off + 1 + j)] == col[rp[node] + j], "row of node %d", node);
        }
        // batches respect the sequential order: a lower-numbered neighbour sits in an earlier batch
        for (int64_t i = 0; i < N; ++i)
            for (int32_t j = rp[i]; j < rp[i + 1]; ++j)
                if (col[j] < i) CHECK(level[(size_t)col[j]] < level[(size_t)i], "dependency %d -> %lld", col[j], (long long)i);
        CHECK(nb >= (N > 0) && nl >= (N > 0), "counts");
    }
    // ---- rls_graph_sweep_batches
    {
        Exact<int32_t> flagged((size_t)N + 1);
        int64_t nb = -1;
        const int32_t mn = (int32_t)(1 + rng() % 64), me = (int32_t)(1 + rng() % 1000);
        CHECK(rls_graph_sweep_batches(rp, col, N, mn, me, flagged.p, &nb) == RLS_OK, "%s", rls_last_error_string());
        CHECK(((uint32_t)flagged[(size_t)N] & 0x7fffffffu) == (uint32_t)rp[N], "end offset");
    }
    // ---- rls_graph_ell: sizing call, then an exactly-sized table
    {
        const int64_t groups = (N + 63) / 64;
        Exact<int32_t> ptr((size_t)groups + 1);
        int64_t total = -1;
        CHECK(rls_graph_ell(rp, col, N, ptr.p, nullptr, 0, &total) == RLS_OK, "%s", rls_last_error_string());
        Exact<int32_t> ell((size_t)total);
        CHECK(rls_graph_ell(rp, col, N, ptr.p, ell.p, total, &total) == RLS_OK, "%s", rls_last_error_string());
        CHECK(ptr[(size_t)groups] == total, "ell_ptr end");
        for (int64_t gq = 0; gq < groups; ++gq) {
            const int64_t rounds = (ptr[(size_t)gq + 1] - ptr[(size_t)gq]) / 64;
            for (int64_t l = 0; l < 64; ++l) {
                // a lane's column = its node's neighbours in the builder's (bank-spreading) order + the node itself as padding:
                // the same multiset as the CSR row, nothing else
                const int64_t node = gq * 64 + l;
                std::vector<int32_t> have, want;
                for (int64_t k = 0; k < rounds; ++k) have.push_back(ell[(size_t)(ptr[(size_t)gq] + 64 * k + l)]);
                if (node < N) {
                    for (int64_t j = rp[node]; j < rp[node + 1]; ++j) want.push_back(col[j]);
                    while ((int64_t)want.size() < rounds) want.push_back((int32_t)node);
                    std::sort(have.begin(), have.end());
                    std::sort(want.begin(), want.end());
                    CHECK(have == want, "ell column of node %lld", (long long)node);
                } else {
                    for (int32_t v : have) CHECK(v >= 0 && v < std::max<int64_t>(N, 1) + 64, "ell padding %d", v);
                }
            }
        }
        if (total > 0) CHECK(rls_graph_ell(rp, col, N, ptr.p, ell.p, total - 1, &total) != RLS_OK, "a short table must be refused");
    }
    // ---- rls_graph_sweep_levels (N < 2^20, degrees < 4096)
    if (g.max_deg < 4096) {
        int64_t ng = -1, tot = -1;
        CHECK(rls_graph_sweep_levels(rp, col, N, nullptr, 0, nullptr, 0, &ng, &tot) == RLS_OK, "%s", rls_last_error_string());
        Exact<int32_t> lvp((size_t)ng + 1), lvd((size_t)tot);
        CHECK(rls_graph_sweep_levels(rp, col, N, lvp.p, ng + 1, lvd.p, tot, &ng, &tot) == RLS_OK, "%s", rls_last_error_string());
        std::vector<char> seen((size_t)N, 0);
        for (int64_t q = 0; q < ng; ++q) {
            const int64_t off = (uint32_t)lvp[(size_t)q] & 0x3fffffffu, end = (uint32_t)lvp[(size_t)q + 1] & 0x3fffffffu;
            CHECK(off + 64 <= end && end <= tot, "group %lld bounds", (long long)q);
            const bool hub = ((uint32_t)lvp[(size_t)q] >> 30) & 1;
            if (hub) {
                const int32_t node = lvd[(size_t)off];
                CHECK(node >= 0 && node < N && !seen[(size_t)node], "hub node");
                seen[(size_t)node] = 1;
            } else {
                for (int l = 0; l < 64; ++l) {
                    const int32_t w = lvd[(size_t)(off + l)], node = w & 0xfffff, lg = (w >> 28) & 7;
                    if (node < N && (l & ((1 << lg) - 1)) == 0) {          // the first lane of a row's lanes
                        CHECK(!seen[(size_t)node], "node %d twice", node);
                        seen[(size_t)node] = 1;
                    }
                }
            }
        }
        for (int64_t i = 0; i < N; ++i) CHECK(seen[(size_t)i], "node %lld missing from the level schedule", (long long)i);
        if (tot > 0) {
            int64_t a, b;
            CHECK(rls_graph_sweep_levels(rp, col, N, lvp.p, ng + 1, lvd.p, tot - 1, &a, &b) != RLS_OK, "a short table must be refused");
        }
    }
    // ---- rls_mcpg_visit_levels (degrees < 1024) on a random visiting order and on the degree-descending one
    if (g.max_deg < 1024) {
        for (int pass = 0; pass < 2; ++pass) {
            std::vector<int32_t> order((size_t)N);
            for (int64_t i = 0; i < N; ++i) order[(size_t)i] = (int32_t)i;
            if (pass == 0) std::shuffle(order.begin(), order.end(), rng);
            else std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return rp[a + 1] - rp[a] > rp[b + 1] - rp[b]; });
            int64_t ng = -1, tot = -1;
            CHECK(rls_mcpg_visit_levels(rp, col, N, order.data(), nullptr, 0, nullptr, 0, &ng, &tot) == RLS_OK, "%s", rls_last_error_string());
            Exact<int32_t> lvp((size_t)ng + 1), lvd((size_t)tot);
            CHECK(rls_mcpg_visit_levels(rp, col, N, order.data(), lvp.p, ng + 1, lvd.p, tot, &ng, &tot) == RLS_OK, "%s", rls_last_error_string());
            for (int64_t q = 0; q < ng; ++q) {
                const int64_t off = (uint32_t)lvp[(size_t)q] & 0x3fffffffu, end = (uint32_t)lvp[(size_t)q + 1] & 0x3fffffffu;
                CHECK(off + 128 <= end && end <= tot, "visit group %lld bounds", (long long)q);
            }
            if (N > 1) {                      // a non-permutation is refused, not read out of bounds
                order[0] = order[1];
                CHECK(rls_mcpg_visit_levels(rp, col, N, order.data(), nullptr, 0, nullptr, 0, &ng, &tot) != RLS_OK, "duplicate order entry");
            }
        }
    }
}

static void run_oracle(const Graph& g, std::mt19937_64& rng) {
    const int64_t N = g.n, E = (int64_t)g.eu.size(), B = 1 + (int64_t)(rng() % 9);
    Exact<uint8_t> xs((size_t)(B * N));
    for (size_t i = 0; i < xs.n; ++i) xs[i] = (uint8_t)(rng() & 1);
    Exact<int64_t> obj((size_t)B), last((size_t)B), act((size_t)B), rew((size_t)B), before((size_t)B), cd((size_t)(B * N));
    const int32_t* eu = E ? g.eu.data() : nullptr;
    const int32_t* ev = E ? g.ev.data() : nullptr;
    orc_maxcut_obj(xs.p, B, N, eu, ev, E, 0, obj.p);
    orc_node_cutdeg(xs.p, B, N, g.erowptr.data(), ev, cd.p);
    for (int64_t b = 0; b < B; ++b) {
        int64_t s = 0;
        for (int64_t i = 0; i < N; ++i) s += cd[(size_t)(b * N + i)];
        CHECK(s == obj[(size_t)b], "sum of stored-adjacency cut degrees == cut");
        last[(size_t)b] = before[(size_t)b] = obj[(size_t)b];
        act[(size_t)b] = (int64_t)(rng() % (uint64_t)N);
    }
    orc_step_u8(xs.p, B, N, act.p, eu, ev, E, 0, last.p, rew.p);
    orc_maxcut_obj(xs.p, B, N, eu, ev, E, 0, obj.p);
    for (int64_t b = 0; b < B; ++b)
        CHECK(obj[(size_t)b] == last[(size_t)b] && rew[(size_t)b] == last[(size_t)b] - before[(size_t)b], "step keeps the objective");
    if (N <= 700) {
        orc_greedy_sweep(xs.p, B, N, eu, ev, E, 0, last.p);
        orc_maxcut_obj(xs.p, B, N, eu, ev, E, 0, obj.p);
        for (int64_t b = 0; b < B; ++b) CHECK(obj[(size_t)b] == last[(size_t)b], "sweep keeps the objective");
    }
    const int64_t T = 2 + (int64_t)(rng() % 30);
    Exact<float> dist((size_t)(T * T)), len((size_t)B);
    for (size_t i = 0; i < dist.n; ++i) dist[i] = (float)(rng() % 1000) / 7.0f;
    Exact<int64_t> perm((size_t)(B * T));
    for (int64_t b = 0; b < B; ++b) {
        for (int64_t k = 0; k < T; ++k) perm[(size_t)(b * T + k)] = k;
        std::shuffle(perm.p + b * T, perm.p + (b + 1) * T, rng);
    }
    orc_tsp_tour_length(dist.p, T, perm.p, B, len.p);
}

// every planner over random shapes (sizes up to past every LDS limit, every flag, random knobs): no overflow, no plan past the LDS
static void run_planners(std::mt19937_64& rng) {
    rls::TileShape s{};
    s.N = 1 + (int64_t)(rng() % 200000); s.B = 1 + (int64_t)(rng() % (1 << 17)); s.E = (int64_t)(rng() % (1 << 25));
    s.nnz = 2 * s.E; s.G = (int64_t)(rng() % (s.N / 32 + 2)); s.spin_bytes = rng() & 1 ? 1 : 4; s.max_degree = (int32_t)(rng() % 70000);
    const uint64_t f = rng();
    s.rows_aligned = f & 1; s.out16 = f & 2; s.mask_bits = f & 4; s.minmax = f & 8; s.weighted = (f & 48) == 48;
    s.has_levels = f & 64; s.has_batches = f & 128; s.has_ell = f & 256; s.col4 = f & 512; s.cus = 1 + (int)(rng() % 512);
    if (f & 1024) rls_tuning_set(f & 2048 ? "RLS_NARROW_TILE" : "RLS_NS_TILE32", (int64_t)(rng() % 4));
    const rls::LaunchPlan plans[] = {rls::plan_obj(s), rls::plan_propose_accept(s), rls::plan_greedy_sweep(s), rls::plan_node_stats(s, 0),
                                     rls::plan_node_stats(s, 1), rls::plan_node_stats(s, 2)};
    for (const rls::LaunchPlan& p : plans)
        CHECK(p.form == rls::PF_UNSUPPORTED ? p.err == RLS_EUNSUPPORTED && p.msg[0] != 0 : p.lds <= (size_t)rls::kLdsBytes && p.grid >= 1 && p.block >= 64,
              "plan form %d lds %zu grid %u block %u", p.form, p.lds, p.grid, p.block);
    rls_tuning_unset(nullptr);
    // the TSP planner: sizes past every limit (the step's 10 240, K13's 5088), any K
    const int64_t tn = 1 + (int64_t)(rng() % 12000);
    const int32_t tk = (int32_t)(rng() % 300);
    const rls::TspForm forms[] = {rls::tsp_plan_tour_length(tn), rls::tsp_plan_swap_delta(tn, tk, (f & 4096) != 0), rls::tsp_plan_step(tn),
                                  rls::tsp_plan_2opt_best(tn * 4, (f & 8192) != 0), rls::tsp_plan_rand_perms(tn)};
    for (const rls::TspForm& p : forms)
        CHECK(p.err == RLS_EUNSUPPORTED || (p.err == RLS_OK && p.lds <= (size_t)rls::kLdsBytes && p.block >= 64 && p.waves * 64 == p.block &&
                                            (!p.tab8 || p.lds_d)),
              "TSP form N %lld K %d err %d lds %zu block %d waves %d", (long long)tn, tk, p.err, p.lds, p.block, p.waves);
}

// the local-search planner over random shapes (N up to past the narrow tile, any layout flags, scratch around what the query asks for,
// random policy knobs): a plan is a refusal with a text or launches that fit LDS; what the host queries answer -- supported, scratch
// bytes, slices -- is what the plans do with it; rls_maxcut_ls_propose's plan is rls_maxcut_ls_rounds' with one draw
static void run_ls_plans(std::mt19937_64& rng) {
    using namespace rls;
    static const char* kKnobs[] = {"RLS_LS_WAVES", "RLS_LS_SLICES", "RLS_LS_PER_ROUND", "RLS_LS_APPLY32", "RLS_LS_SD_GLOBAL", "RLS_NARROW_TILE", "RLS_SWEEP_NO_LEVELS"};
    const uint64_t f = rng();
    if (f & 1) rls_tuning_set(kKnobs[rng() % 7], (int64_t)(rng() % 9));
    LsShape s{};
    s.N = f & 2 ? 1 + (int64_t)(rng() % 170000) : 1 + (int64_t)(rng() % 26000); s.B = 1 + (int64_t)(rng() % (1 << 17)); s.E = (int64_t)(rng() % (1 << 25));
    s.G = (int64_t)(rng() % (s.N / 32 + 2)); s.ws_bytes = f & 4 ? 1 : 2; s.num_spin = (int)(rng() % 18); s.num_draws = 1 + (int)(rng() % 9);
    s.ws_pitch = s.N + (int64_t)(rng() % 17); s.max_degree = (int)(rng() % 600); s.cus = 1 + (int)(rng() % 512);
    s.weighted = (f & 24) == 24; s.has_levels = f & 32; s.has_batches = f & 64; s.x_aligned = (f & 128) && (s.N & 3) == 0; s.noise16 = f & 256;
    s.pitch_ok = ((s.ws_pitch * s.ws_bytes) & 15) == 0; s.scratch_ok = (f & 1536) != 0;
    const size_t ask = ls_scratch_bytes(s);
    s.scratch_bytes = f & 2048 ? ask : (f & 4096 ? (ask ? ask - 1 : 0) : (size_t)(rng() % (2 * ask + 2)));
    const LsTile t = ls_tile(s);
    const LsPlan plans[] = {plan_ls_fused(s), plan_ls_threshold(s), plan_ls_propose(s), plan_ls_rounds(s)};
    for (const LsPlan& p : plans) {
        CHECK(p.err == RLS_OK ? p.n >= 1 && p.n <= 2 && p.repeat >= 1 && p.repeat * p.per_launch == (&p == &plans[3] ? s.num_draws : 1)
                              : p.err == RLS_EUNSUPPORTED && p.msg[0] != 0 && p.n == 0, "ls plan N %lld: err %d n %d repeat %d", (long long)s.N, p.err, p.n, p.repeat);
        for (int i = 0; i < p.n; ++i)
            CHECK(p.l[i].lds >= 0 && p.l[i].lds <= kLdsBytes && p.l[i].grid[0] >= 1 && p.l[i].grid[1] >= 1 && p.l[i].grid[1] <= 8 && p.l[i].grid[2] >= 1 &&
                      (p.l[i].kernel == LSK_K6 || p.l[i].block >= 64), "ls launch N %lld kernel %d lds %lld", (long long)s.N, p.l[i].kernel, (long long)p.l[i].lds);
    }
    // the views: the answer of each host query is what the plans do on well-laid-out arguments with the scratch asked for
    LsShape v = s;
    v.pitch_ok = v.noise16 = v.scratch_ok = true; v.x_aligned = (s.N & 3) == 0; v.scratch_bytes = ask;
    CHECK(ls_fused_supported(s) == (plan_ls_fused(v).err == RLS_OK), "fused supported N %lld", (long long)s.N);
    const LsPlan th = plan_ls_threshold(v), all = plan_ls_rounds(v);
    CHECK(th.err != RLS_OK || ((int)th.l[0].grid[1] == t.slices && th.n == (t.slices > 1 ? 2 : 1)), "slices N %lld: %d", (long long)s.N, t.slices);
    if (all.err == RLS_OK && all.l[0].kernel == LSK_MASK && all.l[0].round_words != 0)
        CHECK((int)all.l[0].grid[1] == t.slices && ask >= ls_round_bytes(s) * (size_t)all.per_launch, "mask words N %lld", (long long)s.N);
    if (all.err == RLS_OK && s.num_draws > 1 && !knob_on(KN_LS_PER_ROUND) && ls_round_bytes(s) * (size_t)s.num_draws <= kLsMaxMaskBytes)
        CHECK(all.per_launch == s.num_draws && all.repeat == 1, "all rounds at once N %lld draws %d", (long long)s.N, s.num_draws);
    LsShape one = v;
    one.num_draws = 1; one.scratch_bytes = ls_scratch_bytes(one);
    const LsPlan r1 = plan_ls_rounds(one), pr = plan_ls_propose(one);
    CHECK(ls_rounds_supported(s) == (ls_spin_ok(s) && r1.err == RLS_OK), "rounds supported N %lld", (long long)s.N);
    CHECK(pr.err == r1.err && pr.n == r1.n && pr.repeat == r1.repeat && std::string(pr.msg) == r1.msg, "propose is rounds with one draw, N %lld", (long long)s.N);
    for (int i = 0; i < r1.n; ++i)
        CHECK(pr.l[i].kernel == r1.l[i].kernel && pr.l[i].lds == r1.l[i].lds && pr.l[i].grid[0] == r1.l[i].grid[0] && pr.l[i].grid[1] == r1.l[i].grid[1] &&
                  pr.l[i].sd_lds == r1.l[i].sd_lds && pr.l[i].premask == r1.l[i].premask && pr.l[i].stage == r1.l[i].stage, "propose launch %d, N %lld", i, (long long)s.N);
    if (r1.err == RLS_OK && ls_masked(t.cls)) {      // the rounds run through the mask words: not with a byte less than the query says
        --one.scratch_bytes;
        CHECK(plan_ls_rounds(one).err == RLS_EUNSUPPORTED, "N %lld ran short of scratch", (long long)s.N);
    }
    rls_tuning_unset(nullptr);
}

// the ISCO steps' planner (graph and dense) over random (N, B) up to past every LDS limit, under every combination of its four dev
// knobs: a plan fits LDS, its lists are powers of two of at least 64 entries (or hold every node of a smaller graph, or are the
// forced capacity), 1..8 samples share a workgroup, and only rows of >= 256 nodes in LDS get a workgroup per sample by choice
static void run_isco_plans(std::mt19937_64& rng) {
    const int64_t caps[] = {-1, 16, 64, 1024}, wgs[] = {-1, 0, 1}, grs[] = {-1, 1}, wvs[] = {-1, 1, 4, 8};
    auto set = [](const char* name, int64_t v) { if (v >= 0) rls_tuning_set(name, v); };
    auto pow2 = [](int v) { return v >= 1 && (v & (v - 1)) == 0; };
    for (int k = 0; k < 8; ++k) {
        const int64_t N = k == 0 ? 8 * (1 + (int64_t)(rng() % 40)) : 1 + (int64_t)(rng() % (k < 4 ? 20000 : 100000));
        const int64_t B = 1 + (int64_t)(rng() % (1 << 15));
        const int cus = 1 + (int)(rng() % 512);
        for (int64_t cap : caps) for (int64_t wg : wgs) for (int64_t gr : grs) for (int64_t wv : wvs) {
            set("RLS_ISCO_SEL_CAP", cap); set("RLS_ISCO_FORCE_WG", wg); set("RLS_ISCO_GLOBAL_ROWS", gr); set("RLS_ISCO_WAVES", wv);
            for (int dense = 0; dense < 2; ++dense) {
                const int64_t n = dense ? (N + 7) / 8 * 8 : N;
                const rls::IscoPlan p = rls::isco_plan_step(rls::isco_rows_bytes(n), n, B, cus, dense ? rls::kIscoMinList : 1, !dense);
                int64_t q[8] = {-1, -1, -1, -1, -1, -1, -1, -1};       // the host query answers with the same plan
                CHECK(rls_isco_launch_plan(n, B, cus, dense, q) == RLS_OK && q[0] == p.wg && q[1] == p.grows && q[2] == p.P && q[3] == p.Pw &&
                          q[4] == p.waves && q[5] == (int64_t)p.lds && q[6] == p.err && q[7] == (int64_t)p.need,
                      "rls_isco_launch_plan N %lld B %lld dense %d differs from isco_plan_step", (long long)n, (long long)B, dense);
                if (p.err != RLS_OK) {
                    CHECK(p.err == RLS_EUNSUPPORTED && p.need > (size_t)rls::kLdsBytes, "ISCO plan N %lld refused at %zu B", (long long)n, p.need);
                    continue;
                }
                auto list_ok = [&](int P) { return pow2(P) && (P >= rls::kIscoMinList || P == cap || (!dense && P >= n)); };
                CHECK(p.lds <= (size_t)rls::kLdsBytes && list_ok(p.P) && list_ok(p.Pw) && p.Pw <= p.P && p.waves >= 1 && p.waves <= 8 &&
                          (!p.grows || (p.wg && !dense)) && (!p.wg || p.grows || n >= 256),
                      "ISCO plan N %lld B %lld dense %d knobs %lld %lld %lld %lld: P %d Pw %d waves %d wg %d grows %d lds %zu", (long long)n,
                      (long long)B, dense, (long long)cap, (long long)wg, (long long)gr, (long long)wv, p.P, p.Pw, p.waves, (int)p.wg,
                      (int)p.grows, p.lds);
            }
            rls_tuning_unset(nullptr);
        }
    }
}

// sub_set_sampling's planner over random (S, N, R, top_k, CUs), sizes up to past the node limit and the 32-bit counters: it refuses
// exactly where rls_sub_set_sampling_supported says 0; a plan fits LDS, has a nonzero one-dimensional grid, and its chunks are
// nonempty, disjoint and cover every repeat exactly once
static void run_subset_plans(std::mt19937_64& rng) {
    for (int it = 0; it < 64; ++it) {
        const uint64_t f = rng();
        int64_t S = (f & 7) == 0 ? (int64_t)(rng() % 3) : (int64_t)(rng() % (1 << 17));
        int64_t N = it == 0 ? rls::kSubsetMaxN : (it == 1 ? rls::kSubsetMaxN + 1 : 1 + (int64_t)(rng() % ((f & 8) ? 40000 : 4200)));
        int64_t R = (f & 48) == 0 ? 1 + (int64_t)(rng() % 40) : 1 + (int64_t)(rng() % 70000);
        int64_t top_k = (int64_t)(rng() % (uint64_t)(N + 8));
        if ((f & 0xF00) == 0) R = (f & 0x1000) ? (1ll << 31) : (int64_t)(rng() % 3) - 1;                  // past the counter | 0, -1
        if ((f & 0xF000) == 0) { S = (1ll << 30) + (int64_t)(rng() % 7); R = (1ll << 30); N = 20000; }      // R S N past int64
        if ((f & 0xF0000) == 0) top_k = -1 - (int64_t)(rng() % 5);
        const int cus = 1 + (int)(rng() % 512);
        const int sup = rls_sub_set_sampling_supported(S, N, R, top_k);
        const rls::SubsetPlan p = rls::subset_plan(S, N, R, top_k, cus);
        CHECK((p.err == RLS_OK) == (sup == 1) && (p.err == RLS_OK || p.err == RLS_EUNSUPPORTED), "subset plan S %lld N %lld R %lld k %lld: err %d, supported %d",
              (long long)S, (long long)N, (long long)R, (long long)top_k, p.err, sup);
        CHECK(sup == (S >= 0 && N >= 1 && N <= RLS_SUB_SET_SAMPLING_MAX_NODES && R >= 1 && R < (1ll << 31) && S < (1ll << 31) && top_k >= 0 &&
                      (S == 0 || (__int128)R * S * N <= (__int128)INT64_MAX)), "subset supported S %lld N %lld R %lld k %lld: %d", (long long)S,
              (long long)N, (long long)R, (long long)top_k, sup);
        if (p.err != RLS_OK) continue;
        CHECK(p.lds == rls::subset_lds_bytes(N) && p.lds <= (size_t)rls::kLdsBytes && (p.block == 256 || p.block == 512 || p.block == 1024) &&
                  (size_t)rls::kLdsBytes / p.lds * (size_t)p.block >= 1024, "subset plan N %lld: lds %zu block %d", (long long)N, p.lds, p.block);
        CHECK(p.repeats >= 1 && p.chunks >= 1 && (p.chunks - 1) * p.repeats < R && p.chunks * p.repeats >= R,
              "subset plan R %lld: %lld chunks of %lld repeats", (long long)R, (long long)p.chunks, (long long)p.repeats);
        std::vector<char> covered((size_t)R, 0);
        if (R <= 4096)
            for (int64_t c = 0; c < p.chunks; ++c)
                for (int64_t r = c * p.repeats; r < std::min(R, (c + 1) * p.repeats); ++r) CHECK(!covered[(size_t)r]++, "repeat %lld twice", (long long)r);
        if (R <= 4096) for (int64_t r = 0; r < R; ++r) CHECK(covered[(size_t)r] == 1, "repeat %lld not covered", (long long)r);
        CHECK(S == 0 || (S * p.chunks >= 1 && S * p.chunks < (1ll << 31)), "subset grid %lld x %lld", (long long)S, (long long)p.chunks);
    }
}

// the MaxSAT level schedule (rls_maxsat_visit_levels) over random formulas: k-SAT with repeated variables, long clauses, empty
// clauses, a hub variable, weighted or not, a random visiting order -- sized, then filled into buffers of exactly that size; every
// entry points inside the tile, every variable sits in exactly one lane, a buffer one word short is refused
static void run_maxsat(std::mt19937_64& rng, int it) {
    const int nvar = 1 + (int)(rng() % (it % 7 == 0 ? 3000 : 90)), M = (int)(rng() % (5 * (uint64_t)nvar + 2));
    const bool weighted = rng() % 3 == 0;
    std::vector<int32_t> cp{0}, lit, w, order((size_t)nvar);
    for (int c = 0; c < M; ++c) {
        int k = (int)(rng() % 7);
        if (rng() % 50 == 0) k = 40 + (int)(rng() % 30);
        for (int j = 0; j < k; ++j) {
            const int v = (j == 0 && it % 5 == 0) ? 0 : (int)(rng() % (uint64_t)nvar);
            lit.push_back((v + 1) * ((rng() & 1) ? 1 : -1));
        }
        cp.push_back((int32_t)lit.size());
        w.push_back(1 + (int32_t)(rng() % 20));
    }
    for (int i = 0; i < nvar; ++i) order[(size_t)i] = i;
    for (int i = nvar - 1; i > 0; --i) std::swap(order[(size_t)i], order[(size_t)(rng() % (uint64_t)(i + 1))]);
    const int32_t* wp = weighted ? w.data() : nullptr;
    int64_t ng = 0, tot = 0, ng2 = 0, tot2 = 0;
    CHECK(rls_maxsat_visit_levels(cp.data(), lit.data(), wp, nvar, M, order.data(), nullptr, 0, nullptr, 0, &ng, &tot) == RLS_OK, "maxsat sizing: %s",
          rls_last_error_string());
    std::vector<int32_t> lvp((size_t)ng + 1), lvd((size_t)tot);
    CHECK(rls_maxsat_visit_levels(cp.data(), lit.data(), wp, nvar, M, order.data(), lvp.data(), (int64_t)lvp.size(), lvd.data(), (int64_t)lvd.size(),
                                  &ng2, &tot2) == RLS_OK && ng2 == ng && tot2 == tot, "maxsat fill: %s", rls_last_error_string());
    std::vector<int> seen((size_t)nvar, 0);
    const int64_t B = weighted ? 512 : 256;
    for (int64_t g = 0; g < ng; ++g) {
        const int64_t p0 = (int64_t)(lvp[(size_t)g] & 0xFFFFFF) * 64, p1 = (int64_t)(lvp[(size_t)g + 1] & 0xFFFFFF) * 64;
        CHECK(p0 + 128 <= p1 && p1 + 512 <= tot && (p1 - p0 - 128) % B == 0, "maxsat record %lld", (long long)g);
        for (int l = 0; l < 64; ++l)
            if (lvd[(size_t)(p0 + 2 * l)] < nvar) ++seen[(size_t)lvd[(size_t)(p0 + 2 * l)]];
        for (int64_t b = 0; p0 + 128 + b * B < p1; ++b)
            for (int e = 0; e < 256; ++e)
                CHECK((((uint32_t)lvd[(size_t)(p0 + 128 + b * B + e)] & 0x3FFF8u) >> 3) <= (uint32_t)nvar, "maxsat entry past the tile");
    }
    for (int v = 0; v < nvar; ++v) CHECK(seen[(size_t)v] == 1, "maxsat: variable %d scheduled %d times", v, seen[(size_t)v]);
    std::vector<int32_t> small((size_t)tot - 1);
    CHECK(rls_maxsat_visit_levels(cp.data(), lit.data(), wp, nvar, M, order.data(), lvp.data(), (int64_t)lvp.size(), small.data(),
                                  (int64_t)small.size(), &ng2, &tot2) == RLS_EINVAL, "maxsat: a short buffer was accepted");
    if (!lit.empty()) {
        lit[(size_t)(rng() % lit.size())] = (rng() & 1) ? 0 : nvar + 1;
        CHECK(rls_maxsat_visit_levels(cp.data(), lit.data(), wp, nvar, M, order.data(), nullptr, 0, nullptr, 0, &ng2, &tot2) == RLS_EINVAL,
              "maxsat: a bad literal was accepted");
    }
}

int main(int argc, char** argv) {
    const int iters = argc > 1 ? std::atoi(argv[1]) : 200;
    std::mt19937_64 rng(argc > 2 ? (uint64_t)std::atoll(argv[2]) : 20261003ull);
    CHECK(rls_version() == RLS_ABI_VERSION, "version");
    // argument checks return codes instead of touching memory
    int64_t a = 0, b = 0;
    CHECK(rls_graph_sweep_schedule(nullptr, nullptr, 4, 64, 768, nullptr, nullptr, &a, &b) == RLS_EINVAL, "null rowptr");
    CHECK(rls_last_error_string()[0] != 0, "error text recorded");
    for (int it = 0; it < iters; ++it) {
        const int kind = it < 6 ? it : (int)(rng() % 6);
        Graph g = make_graph(rng, kind);
        run_builders(g, rng);
        run_oracle(g, rng);
        for (int k = 0; k < 50; ++k) run_planners(rng);
        for (int k = 0; k < 50; ++k) run_ls_plans(rng);
        run_isco_plans(rng);
        run_subset_plans(rng);
        run_maxsat(rng, it);
    }
    std::printf("host_sanitize: %d random graphs through the host builders and the C oracle, clean\n", iters);
    return 0;
}
