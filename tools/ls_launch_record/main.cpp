// The host side of csrc/rls_localsearch.hip without a device: linked with an object of that file compiled behind shim.h, this program
// calls its entry points on dummy pointers and prints, per case, every launch (kernel with template arguments, grid, block, LDS,
// arguments: integers by value, pointers by the dummy they point into) and the refusal, as one JSON line.  Cases come on stdin, one
// per line (record.py writes them):
//   entry N B ws_bytes E ws_pitch num_spin num_draws x_off noise_off scratch_mode scratch_off schedule weighted max_degree [KNOB=value ...]
// entry: 0 rls_maxcut_local_search, 1 _ls_threshold, 2 _ls_propose, 3 _ls_rounds.  scratch_mode: 0 none, 1 / 2 what
// rls_maxcut_ls_scratch_bytes asks for one / num_draws rounds, 3 that less one byte.  schedule: 0 CSR, 1 batches, 2 levels.
// Built with -DRECORD_MCPG and an object of csrc/rls_mcpg.hip instead, it records the three MCPG local-search launchers:
//   entry N C spin_bytes out_spin_bytes E weighted max_degree gauge_node [KNOB=value ...]
// entry: 4 rls_mcpg_local_search_levels, 5 rls_mcpg_local_search with the batched visit stream, 6 without.
#include <cxxabi.h>
#include <dlfcn.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sstream>
#include <string>
#include "shim.h"
#include "rls_host.h"

static std::string g_out, g_err;
static const char* kDummies[] = {"0", "x", "ws", "sd", "noise", "th", "obj", "scr", "eu", "ev", "rowptr", "erowptr", "col", "wgt",
                                 "sweep_rowptr", "sweep_stream", "sweep_lv_ptr", "sweep_lv_data", "g", "xs_out", "lv_ptr", "lv_data", "coins", "expected", "order",
                                 "visit", "uniforms", "weights"};
constexpr int kShift = 40;
template <class T = void>
static T* dummy(const char* name, long long off = 0) {
    for (size_t i = 1; i < sizeof(kDummies) / sizeof(*kDummies); ++i)
        if (!strcmp(kDummies[i], name)) return reinterpret_cast<T*>(((uintptr_t)i << kShift) + (uintptr_t)off);
    abort();
}
static std::string name_of(const void* p) {
    const uintptr_t v = (uintptr_t)p, i = v >> kShift, off = v & (((uintptr_t)1 << kShift) - 1);
    if (i >= sizeof(kDummies) / sizeof(*kDummies)) return "?";
    return off ? std::string(kDummies[i]) + "+" + std::to_string(off) : kDummies[i];
}

namespace ls_rec {
void begin(const void* kern, dim3 grid, dim3 block, size_t lds) {
    Dl_info info{};
    std::string name = "?";
    if (dladdr(kern, &info) && info.dli_sname) {
        int st = 0;
        char* d = abi::__cxa_demangle(info.dli_sname, nullptr, nullptr, &st);
        name = st == 0 && d ? d : info.dli_sname;
        free(d);
        int depth = 0;      // "void rls::k<...>(parameters)" -> "rls::k<...>"
        for (size_t i = 0; i < name.size(); ++i) {
            depth += name[i] == '<' ? 1 : name[i] == '>' ? -1 : 0;
            if (name[i] == '(' && depth == 0) { name.resize(i); break; }
        }
        if (name.rfind("void ", 0) == 0) name.erase(0, 5);
    }
    char buf[160];
    snprintf(buf, sizeof buf, "%s[\"%s\",%u,%u,%u,%u,%zu,\"", g_out.empty() ? "" : ",", name.c_str(), grid.x, grid.y, grid.z, block.x * block.y * block.z, lds);
    g_out += buf;
}
static void sep() { if (g_out.back() != '"') g_out += ","; }
void arg_ptr(const void* p) { sep(); g_out += name_of(p); }
void arg_int(long long v) { sep(); g_out += std::to_string(v); }
void end() { g_out += "\"]"; }
}  // namespace ls_rec

namespace rls {
std::atomic<int64_t> g_knobs[KN_COUNT];
int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
int check_launch(const char*) { return 0; }
}  // namespace rls

#ifndef RECORD_MCPG
extern "C" int rls_maxcut_propose_accept(const rls_graph* g, uint8_t* x, int64_t B, const void* mask, int32_t mask_bits, int64_t* obj, void*) {
    ls_rec::record(nullptr, dim3(0, 0, 0), dim3(0), 0, (const void*)dummy("g"), x, B, mask, mask_bits, obj);
    g_out.replace(g_out.rfind("[\"?\""), 4, "[\"rls_maxcut_propose_accept\"");
    return 0;
}
#endif

static const char* kKnobNames[] = {
#define RLS_X(n) #n,
    RLS_KNOB_LIST(RLS_X)
#undef RLS_X
};

int main() {
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        std::istringstream in(line);
#ifdef RECORD_MCPG
        long long entry, N, C, spin, out_spin, E, weighted, max_degree, gauge;
        if (!(in >> entry >> N >> C >> spin >> out_spin >> E >> weighted >> max_degree >> gauge)) continue;
#else
        long long entry, N, B, ws_bytes, E, pitch, num_spin, draws, x_off, noise_off, smode, s_off, sched, weighted, max_degree;
        if (!(in >> entry >> N >> B >> ws_bytes >> E >> pitch >> num_spin >> draws >> x_off >> noise_off >> smode >> s_off >> sched >> weighted >> max_degree)) continue;
#endif
        for (auto& k : rls::g_knobs) k.store(rls::kKnobUnset);
        for (std::string kv; in >> kv;) {
            const size_t eq = kv.find('=');
            int idx = -1;
            for (int i = 0; i < rls::KN_COUNT; ++i) if (kv.substr(0, eq) == kKnobNames[i]) idx = i;
            if (idx < 0 || eq == std::string::npos) { fprintf(stderr, "unknown knob %s\n", kv.c_str()); return 2; }
            rls::g_knobs[idx].store(atoll(kv.c_str() + eq + 1));
        }
        rls_graph g{};
        g.num_nodes = N; g.num_stored_edges = E; g.nnz = 2 * E; g.if_bidirectional = 1; g.max_degree = (int32_t)max_degree;
        g.eu = dummy<int32_t>("eu"); g.ev = dummy<int32_t>("ev"); g.rowptr = dummy<int32_t>("rowptr"); g.erowptr = dummy<int32_t>("erowptr");
        g.col = dummy<int32_t>("col");
        g_out.clear(); g_err.clear();
        int rc = 0;
#ifdef RECORD_MCPG
        const int64_t groups = N / 64 + 3, ent = weighted ? 2 : 1, hdr = weighted ? 5 : 4;
        if (entry == 4)
            rc = rls_mcpg_local_search_levels(&g, dummy("x"), (int)spin, C, dummy("xs_out"), (int)out_spin, C, dummy<int32_t>("lv_ptr"), dummy<int32_t>("lv_data"), groups, 3,
                                              dummy<uint64_t>("coins"), 7, dummy<float>("expected"), nullptr, nullptr);
        else
            rc = rls_mcpg_local_search(&g, dummy("x"), (int)spin, dummy<float>("xs_out"), C, dummy<int32_t>("order"), entry == 5 ? dummy<int32_t>("visit") : nullptr,
                                       ent * g.nnz + (hdr + 1) * N + 3, 3, dummy<float>("uniforms"), 7, weighted ? dummy<int32_t>("weights") : nullptr, gauge,
                                       dummy<float>("expected"), nullptr, nullptr);
        printf("{\"rc\":%d,\"err\":\"%s\",\"l\":[%s]}\n", rc, rc ? g_err.c_str() : "", g_out.c_str());
#else
        g.wgt = weighted ? dummy<int32_t>("wgt") : nullptr;
        if (sched >= 1) { g.sweep_rowptr = dummy<int32_t>("sweep_rowptr"); g.sweep_stream = dummy<int32_t>("sweep_stream"); }
        if (sched >= 2) { g.sweep_lv_ptr = dummy<int32_t>("sweep_lv_ptr"); g.sweep_lv_data = dummy<int32_t>("sweep_lv_data"); g.num_sweep_groups = N / 64 + 3; }
        const long long need = rls_maxcut_ls_scratch_bytes(&g, B, (int32_t)ws_bytes, (int32_t)(smode == 1 ? 1 : draws));
        const long long sbytes = smode == 0 ? 0 : (smode == 3 ? (need > 0 ? need - 1 : 0) : need);
        void* scratch = smode == 0 ? nullptr : dummy("scr", s_off);
        uint8_t* x = dummy<uint8_t>("x", x_off);
        const uint64_t seed = 7;
        const int64_t env_offset = 3;
        switch (entry) {
            case 0: rc = rls_maxcut_local_search(&g, x, B, dummy("ws"), (int32_t)ws_bytes, pitch, dummy<float>("sd"), dummy<float>("noise", noise_off), seed, env_offset,
                                                 8, (int32_t)num_spin, 1, dummy<int64_t>("obj"), 1, nullptr); break;
            case 1: rc = rls_maxcut_ls_threshold(&g, B, dummy("ws"), (int32_t)ws_bytes, pitch, dummy<float>("sd"), seed, env_offset, 2, (int32_t)num_spin,
                                                 dummy<float>("th"), scratch, sbytes, nullptr); break;
            case 2: rc = rls_maxcut_ls_propose(&g, x, B, dummy("ws"), (int32_t)ws_bytes, pitch, dummy<float>("sd"), dummy<float>("th"), seed, env_offset, 2,
                                               dummy<int64_t>("obj"), scratch, sbytes, nullptr); break;
            default: rc = rls_maxcut_ls_rounds(&g, x, B, dummy("ws"), (int32_t)ws_bytes, pitch, dummy<float>("sd"), dummy<float>("th"), seed, env_offset, 2,
                                               (int32_t)draws, dummy<int64_t>("obj"), scratch, sbytes, nullptr); break;
        }
        printf("{\"q\":[%d,%d,%lld,%d],\"sb\":%lld,\"rc\":%d,\"err\":\"%s\",\"l\":[%s]}\n", rls_maxcut_local_search_supported(&g, B, (int32_t)num_spin),
               rls_maxcut_ls_rounds_supported(&g, (int32_t)num_spin), (long long)rls_maxcut_ls_scratch_bytes(&g, B, (int32_t)ws_bytes, (int32_t)draws),
               rls_maxcut_ls_slices(&g, B, (int32_t)ws_bytes), sbytes, rc, rc ? g_err.c_str() : "", g_out.c_str());
#endif
    }
    return 0;
}
