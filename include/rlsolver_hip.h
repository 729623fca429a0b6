/*
 * rlsolver_hip.h -- C ABI of the MI355X (gfx950) combinatorial-optimisation
 * environment engine.
 *
 * The reference (Open-Finance-Lab/RLSolver) has no FFI: its hot path is a set
 * of duck-typed Python classes that launch chains of ATen ops.  Each entry
 * point below replaces one such chain with ONE hand-written HIP kernel; the
 * comment on each names the reference interface it stands in for (file:line
 * relative to the reference root).  The Python classes in rlsolver_amd/ bind
 * these symbols with ctypes (see INTEGRATION.md for the stub a reference
 * maintainer would add).
 *
 * Conventions
 *   - every function returns RLS_OK (0) or a negative RLS_E* code and records a
 *     message retrievable with rls_last_error_string() (thread local);
 *   - no function allocates, frees or synchronises; all work is enqueued on
 *     `stream` (a hipStream_t passed as void*; NULL = the default stream);
 *   - every pointer is a DEVICE pointer owned by the caller unless marked
 *     [host]; sizes are int64_t; tensors are dense row-major;
 *   - "spins" x are one byte per node (torch.bool / uint8, values 0|1),
 *     env-major [B, N], unless the function takes `spin_bytes` (1 = uint8,
 *     4 = float32 holding 0.0f|1.0f, the env_PPO surface);
 *   - B = number of parallel environments ("sims"), N = nodes, E' = edges as
 *     stored by the env (E, or 2E when if_bidirectional).
 *   - graph size: the MaxCut kernels keep a bit tile of the spins in LDS -- 64 envs x N nodes (N <= 20 224) or, past
 *     that and wherever it measures faster, a half tile of 32 envs (N <= ~40 000; csrc/rls_tile32.h).  Larger graphs take
 *     one-env-per-wave forms (N <= 160 000): correct, an order of magnitude slower.  The choice is per launch and changes
 *     no result.
 */
#ifndef RLSOLVER_HIP_H
#define RLSOLVER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RLS_ABI_VERSION 12

enum {
    RLS_OK = 0,
    RLS_EINVAL = -1,      /* bad argument (null pointer, negative size, bad enum) */
    RLS_EUNSUPPORTED = -2,/* valid request outside what the kernels cover (e.g. N too large for LDS) */
    RLS_ELAUNCH = -3,     /* hipLaunchKernel / hipGetLastError reported a failure */
    RLS_ENODEVICE = -4    /* no HIP device visible */
};

/* One shared graph, resident in HBM/L2.  Host struct of device pointers; built
 * by the caller from rlsolver_amd.graph.GraphCSR.  Replaces the per-env index
 * tensors n0_ids/n1_ids/sim_ids [B,E'] int64 of envs/env_L2A.py:46-59 (24*B*E'
 * bytes there; (N+1+2E+2E')*4 bytes here, independent of B). */
typedef struct rls_graph {
    int64_t num_nodes;        /* N */
    int64_t num_stored_edges; /* E' */
    int64_t nnz;              /* entries of the symmetric CSR: 2E less the self loops, which the env graphs drop; the
                               * MCPG / ISCO graphs list a loop twice in its row instead (build_csr keep_loops), so 2E */
    int32_t if_bidirectional; /* result of objective kernels is count / 2 when set */
    int32_t max_degree;       /* an UPPER BOUND on every row length: the largest row of either adjacency (the stored
                               * out-degree counts loops, the symmetric CSR may not); readers use it only as a bound */
    const int32_t* eu;        /* [E'] edge endpoints as stored, sorted by (eu, ev) */
    const int32_t* ev;        /* [E'] */
    const int32_t* erowptr;   /* [N+1] offsets of each node's run in eu/ev (the env's adjacency_indies) */
    const int32_t* rowptr;    /* [N+1] symmetric CSR */
    const int32_t* col;       /* [nnz] */
    const int32_t* wgt;       /* [nnz] integer edge weights or NULL (= all ones) */
    const int32_t* sweep_rowptr; /* [N+1] offsets into sweep_stream per schedule position, bit 31 = first position
                                  * of a batch (rls_graph_sweep_schedule), or NULL: single-wave sweep */
    const int32_t* sweep_stream; /* [nnz+N] per schedule position: node id, then its neighbours; or NULL */
    /* Lane-per-node slabs of the two adjacencies (rls_graph_ell), or NULL: for the 64-node group g, entries
     * ell_ptr[g] + 64 k + l = k-th neighbour of node 64 g + l, or that node itself past the end of its row. */
    const int32_t* ell_sym_ptr;  /* [ceil(N/64)+1]   symmetric CSR (rowptr/col): K3 */
    const int32_t* ell_sym;
    const int32_t* ell_st_ptr;   /* [ceil(N/64)+1]   adjacency as stored (erowptr/ev): K2, local-search weights */
    const int32_t* ell_st;
    /* Level-parallel form of the sweep schedule (rls_graph_sweep_levels), or NULL / 0 */
    const int32_t* sweep_lv_ptr; /* [num_sweep_groups+1] offset of each 64-lane group in sweep_lv_data, bit 31 = first group of a level, bit 30 = hub group */
    const int32_t* sweep_lv_data;
    int64_t num_sweep_groups;
} rls_graph;

int rls_version(void);
const char* rls_last_error_string(void);
/* Number of HIP devices visible (0 on a CPU-only host; never an error). */
int rls_device_count(void);

/* [host] Tuning table (ABI v11).  Which tile form / wave count / store policy a launch takes is decided per launch from
 * its shapes; every such choice can be FORCED by name ("RLS_K1_TILE32", "RLS_STEP_CHASE", ... -- rls_tuning_name
 * enumerates them; the "RLS_" prefix is optional) for A/B measurements and for the forced-form parity tests.  Forcing a
 * form never changes a result.  The production library reads no environment variable; only a -DRLS_DEV build seeds this
 * table from the environment once, when it is loaded.  The reference has no counterpart (it has no launch policies).
 * rls_tuning_unset(NULL) clears every entry.  Process-wide, not per stream. */
int rls_tuning_set(const char* name, int64_t value);
int rls_tuning_unset(const char* name);
int rls_tuning_get(const char* name, int64_t* value, int32_t* is_set);
int rls_tuning_name(int32_t index, const char** name);   /* index 0 .. until RLS_EINVAL */

/* [host] Level schedule of the sequential greedy sweep (envs/env_L2A.py:109-116 visits i = 0..N-1 and every
 * decision sees the flips of the earlier nodes).  level(i) = 1 + max level of i's lower-numbered neighbours:
 * nodes of one level are pairwise non-adjacent, all earlier neighbours of a node sit in lower levels and all
 * later ones in higher levels, so deciding level after level (any order inside a level) gives exactly the
 * sequential result.  Positions are nodes sorted by (level, id); a level is cut into batches of <= max_nodes
 * nodes and <= max_entries stream entries (what the kernels' LDS ring can hold).
 * rowptr/col: HOST symmetric CSR.  Outputs (host): rowptr_flagged [N+1] = offset of each position's run in
 * `stream`, bit 31 set on the first position of a batch; stream [nnz+N] = node id followed by its neighbours,
 * position after position.  Upload both and store the device pointers in rls_graph.sweep_rowptr /
 * sweep_stream. */
int rls_graph_sweep_schedule(const int32_t* rowptr, const int32_t* col, int64_t N, int32_t max_nodes,
                             int32_t max_entries, int32_t* rowptr_flagged, int32_t* stream, int64_t* num_batches,
                             int64_t* num_levels);

/* [host] The level schedule of rls_graph_sweep_schedule in lane-per-node form: the nodes of a level, longest rows
 * first, in groups of 64 LANES.  A group costs its longest lane and the waves meet at every level boundary, so a row
 * too long for the level's cap (none / 32 / 16 / 8 entries per lane, chosen per level by an instruction-count
 * estimate; never more than 64) takes L = 2, 4 or 8 ADJACENT lanes, lane j of them holding neighbours j, j + L, ...;
 * the kernel adds the lanes' counters before the compare.  Group record in lv_data:
 *     64 words  node | (deg / 2) << 20 | log2 L << 28      (node = N on idle lanes)
 *     per block of 8 rounds, 2 slabs of [64 lanes][4 rounds] (ABI v11: a lane fetches a block in two 16-byte loads) --
 *     round r of lane l at 64 + 512 (r / 8) + 256 ((r / 4) % 2) + 4 l + r % 4:
 *               8 nb                                       (byte offset of the neighbour's word in the tile; the node's
 *                                                           own where the lane's share of the row has ended, 8 N on idle lanes)
 * with rounds = the group's longest lane rounded up to a multiple of 8; the table ends in sixteen spare rows (counted in
 * *total) so that a group's first two blocks can be read unguarded.  A wave decides a whole group at once on 64-env
 * words: bit-sliced count of differing neighbours, bit-sliced compare with deg/2, XOR of the flip mask into
 * the node's word -- bit-identical to the sequential pass (see rls_graph_sweep_schedule).
 * A row of 256 or more entries (a hub) is a group of its own, the first of its level, with lane = neighbour:
 *     64 words  [0] = node, [1] = degree, N elsewhere
 *     rounds (a multiple of 8) in the same block layout: 8 nb, neighbour e in round e / 64 of lane e % 64, the node's own
 *     offset past its end
 * lv_ptr [host, groups+1] (bit 31 = first group of a level, bit 30 = hub group); lv_data [host, capacity] or NULL to size
 * (*num_groups, *total).  Needs N < 2^20 and max degree < 4096. */
int rls_graph_sweep_levels(const int32_t* rowptr, const int32_t* col, int64_t N, int32_t* lv_ptr, int64_t ptr_capacity,
                           int32_t* lv_data, int64_t data_capacity, int64_t* num_groups, int64_t* total);

/* [host] Lane-per-node ("ELL") slabs of a CSR adjacency for the bit-sliced per-node kernels: nodes in groups of
 * 64; group g holds max-degree-in-group rounds of 64 entries, every lane's column = the neighbours of its node in an
 * order chosen by the builder (the node itself where its row is shorter: x_i ^ x_i contributes nothing) -- each round's 32 words
 * of a half-wave are spread over the LDS bank classes n mod 32 as far as the rows allow; consumers must not rely on an order.  ell_ptr [host, G+1] with
 * G = ceil(N/64); ell [host, capacity] or NULL to only compute *total (= ell_ptr[G]) for sizing. */
int rls_graph_ell(const int32_t* rowptr, const int32_t* col, int64_t N, int32_t* ell_ptr, int32_t* ell,
                  int64_t capacity, int64_t* total);

/* [host] Cut the node order 0..N-1 into maximal runs of pairwise NON-adjacent consecutive nodes
 * (<= max_nodes nodes and <= max_entries CSR entries each).  The greedy sweep may decide the nodes of
 * a run in parallel with results identical to the sequential pass of envs/env_L2A.py:109-116.
 * rowptr/col: HOST symmetric CSR; rowptr_flagged [host, N+1] = rowptr with bit 31 set on the first
 * node of each run.  (Used for visiting orders other than 0..N-1: the MCPG visit stream, methods/MCPG.py.) */
int rls_graph_sweep_batches(const int32_t* rowptr, const int32_t* col, int64_t N, int32_t max_nodes,
                            int32_t max_entries, int32_t* rowptr_flagged, int64_t* num_batches);


/* ------------------------------------------------------------------ MaxCut */

/* K1  EnvMaxcut.calculate_obj_values(xs, if_sum=True)  envs/env_L2A.py:54-66
 *     (= env_MCPG.py:54-66, env_PPO.py:108-121, env_k_spin.py:246-258).
 * obj[b] = #{(u,v) in stored edges : x[b,u] != x[b,v]}  (// 2 if bidirectional). */
int rls_maxcut_obj(const rls_graph* g, const void* x, int spin_bytes,
                   int64_t B, int64_t* obj, void* stream);

/* K1' calculate_obj_values(xs, if_sum=False): cutmask[b,e] = x[b,eu[e]] ^ x[b,ev[e]]
 *     as bool bytes [B,E'].  envs/env_L2A.py:61 */
int rls_maxcut_edge_cut_mask(const rls_graph* g, const uint8_t* x, int64_t B,
                             uint8_t* cutmask, void* stream);

/* K2  EnvMaxcut.calculate_obj_values_for_loop(xs, if_sum=False)  env_L2A.py:68-80
 * cutdeg[b,i] = #{j in adj(i) : x[b,j] != x[b,i]} where adj = the env's stored
 * adjacency (out-neighbours only when !if_bidirectional).  int64 [B,N]. */
int rls_maxcut_node_cutdeg(const rls_graph* g, const uint8_t* x, int64_t B,
                           int64_t* cutdeg, void* stream);

/* K3  all-node single-flip gain: delta[b,i] = obj(flip_i(x_b)) - obj(x_b)
 *     = sum_{j in N(i)} w_ij * (x_i == x_j ? +1 : -1), int32 [B,N].
 * Replaces autograd of the energy (envs/env_ISCO.py:51-63), dense
 * matmul(W,s)*s (ECO_S2V/src/envs/spinsystem_PECO.py:661) and the scatter_add
 * form (S2V_PPO/env.py:84-100). */
int rls_maxcut_delta_all(const rls_graph* g, const uint8_t* x, int64_t B,
                         int32_t* delta, void* stream);

/* K4  gym step: env_PPO.EnvMaxcut.step(action)  envs/env_PPO.py:92-106.
 * For every env b: a = action[b]; x_out[b,:] = x_in[b,:] with node a flipped;
 * d = cut gain of that flip; obj[b] += d (in/out, int32); reward[b] = (float)d;
 * cur[b] = (float)obj[b] if cur != NULL; done[b] = done_value if done != NULL.
 * x_out may equal x_in (in-place: only the flipped byte is written, O(deg)
 * traffic); otherwise the whole next state is emitted (2N + 20 B / env-step,
 * the headline byte accounting of SURVEY.md section 8d).  An action outside
 * [0, N) leaves its env untouched and yields reward = NaN (the reference raises). */
int rls_maxcut_step(const rls_graph* g, const void* x_in, void* x_out, int spin_bytes,
                    int64_t B, const int64_t* action, int32_t* obj,
                    float* reward, float* cur, float* done, float done_value,
                    void* stream);

/* [host] The block of runs that workgroup `block` of a one-shot grid of `nblocks` workgroups works on in rls_maxcut_step's
 * write-through form (csrc/rls_step_plan.h, the function the kernels call): order 0 = forward (the block itself), 1 = xcd-fwd
 * (the workgroups with equal block % 8 take one contiguous range).  A bijection on [0, nblocks) for every nblocks; nothing is
 * launched, no device is needed -- what tests pin the map with.  Additive (ABI 12). */
int rls_maxcut_step_block(int32_t order, int64_t block, int64_t nblocks, int64_t* vblock);

/* K5  greedy single-flip sweep ("addition" loop)  envs/env_L2A.py:109-116,
 *     methods/LocalSearch.py:77-83:  for i in 0..N-1: flip i if the cut does
 *     not decrease (ties accept, update_xs_by_vs uses ge, util_read_data.py:199).
 * x [B,N] and obj [B] (int64) are updated in place.  PRECONDITION: obj[b] == cut(x[b]) on entry.  The accept rule itself works on
 * gains (flip i iff its gain >= 0) and does not read obj; what is written back differs by kernel form -- the level-parallel form
 * (the one every unweighted graph with a level schedule takes) counts the cut of the swept tile once and OVERWRITES obj with it,
 * the stream / generic forms ADD the accepted gains to the incoming obj.  The two agree exactly when the precondition holds, which
 * is how every caller on the path uses it (envs/env_L2A.py:91-92 computes good_vs first); a stale or offset obj gives a
 * form-dependent result and is a caller error.  One sequential O(E) pass per env instead of N full objective evaluations. */
int rls_maxcut_greedy_sweep(const rls_graph* g, uint8_t* x, int64_t B,
                            int64_t* obj, void* stream);

/* K6  one multi-flip proposal round of local_search_inplace  envs/env_L2A.py:102-107
 *     (= methods/LocalSearch.py:71-75):  xs = good_xs.clone(); xs[mask] = ~xs[mask];
 *     vs = calculate_obj_values(xs); update_xs_by_vs(good_xs, good_vs, xs, vs).
 * mask uint8 [B,N] is the caller's spin_rand.gt(thresh) (the noise and the
 * kthvalue threshold stay torch ops so they consume torch's generator exactly as
 * the reference does).  x/obj (int64) are updated in place: rows whose proposal
 * has cut >= obj[b] take the proposal.
 * mask_bits != 0: the mask is bit-packed, uint64 [ceil(B/64), N], bit e of word (t, n) = env 64 t + e at node n (bits of envs >= B
 * zero) -- the tile the kernel works on, N / 8 bytes per env instead of N (graphs within the 64-env tile, N <= 20 224, or the
 * half tile of 32 envs, N <= 40 448, which takes the matching dword of each word). */
int rls_maxcut_propose_accept(const rls_graph* g, uint8_t* x, int64_t B, const void* mask, int32_t mask_bits,
                              int64_t* obj, void* stream);

/* Pre-pass of the fused local search  envs/env_L2A.py:90-94 (methods/LocalSearch.py:64-65):
 *   ws[b,i] = n0_num_n1[i] - mult * cutdeg[b,i]   (stored adjacency; exact)
 *   ws_minmax[0][i] = min_b ws[b,i],  ws_minmax[1][i] = max_b ws[b,i]   (int32 [2][N], or NULL: not wanted)
 * mult = 1 for local_search_inplace in both env flavours (bidirectional: 2 * (cutdeg / 2)),
 * 2 for LocalSearch.random_search on a unidirectional env.  ws is ws_bytes = 1 | 2 | 4 bytes per entry (int8 /
 * int16 / int32 [B,N]): |ws| <= max(1, mult - 1) * max degree, and the fused kernel re-reads ws once per proposal
 * round, so the narrowest type that holds the graph's degrees is what keeps that kernel off the HBM roofline
 * (RLS_EINVAL when the range does not fit).  The reference's ws_std = max - min over the batch (:93) is
 * ws_minmax[1] - ws_minmax[0]: the tiles fold their extremes in with atomics that fire only where they improve the
 * table (the table is initialised here, also when B = 0). */
int rls_maxcut_ls_weights(const rls_graph* g, const uint8_t* x, int64_t B, int32_t mult, void* ws, int32_t ws_bytes,
                          int64_t ws_pitch, int32_t* ws_minmax, void* stream);

/* K2+K6+K5 fused: EnvMaxcut.local_search_inplace  envs/env_L2A.py:87-116 (first_draw_proposes = 0)
 * and the body of LocalSearch.random_search  methods/LocalSearch.py:53-83 (first_draw_proposes = 1)
 * in one kernel, the 64-env tile resident in LDS throughout:
 *   thresh[b] = kthvalue(ws[b,:] + noise[0,b,:] * rd_std, k = N - num_spin)
 *   for t in rounds: mask = (ws + noise[t] * rd_std) > thresh; proposal = x ^ mask;
 *                    rows whose proposal has cut >= obj take it                     (:98-107)
 *   greedy single-flip sweep (:109-116)
 * ws int8 / int16 [B,N] (ws_bytes = 1 | 2, as rls_maxcut_ls_weights wrote it) = the reference's
 * n0_num_n1 - k * cutdeg  (exact integer), rd_std f32 [N] = (max_b ws - min_b ws) * noise_std  -- a whole-batch
 * statistic, hence the pre-pass's ws_minmax.
 * noise f32 [num_iters + 1 - first_draw_proposes, B, N] = the randn_like draws in call order (test
 * mode: bit-exact against the reference) or NULL = in-kernel Philox + Box-Muller keyed by
 * (seed, env_offset + b, node, round).  obj int64 [B]: in/out, or out only when compute_obj != 0
 * (the reference's good_vs.shape == () case).  Unweighted graphs, max degree <= 512,
 * num_spin <= 15, rows of x / noise that start 4-byte aligned on 16-byte bases (N % 4 == 0).  ws is read in 16-byte pieces:
 * its rows sit ws_pitch ENTRIES apart (0 = N) and ws_pitch * ws_bytes must be a multiple of 16 on a 16-byte base -- the layout
 * rls_maxcut_ls_weights writes with a padded pitch -- so that no piece leaves its row; an exactly sized [B, N] array whose rows
 * are not 16-byte multiples is refused, never over-read.  RLS_EUNSUPPORTED
 * otherwise (callers take rls_maxcut_ls_threshold + rls_maxcut_ls_rounds, or K2 / K6 / K5). */
int rls_maxcut_local_search(const rls_graph* g, uint8_t* x, int64_t B, const void* ws, int32_t ws_bytes, int64_t ws_pitch,
                            const float* rd_std, const float* noise, uint64_t seed, int64_t env_offset, int32_t num_iters,
                            int32_t num_spin, int32_t first_draw_proposes, int64_t* obj, int32_t compute_obj,
                            void* stream);

/* 1 when rls_maxcut_local_search covers this graph / batch / num_spin (the same test its launcher applies: the
 * 8- or 4-wave LDS layout must fit 160 KB), else 0 -- callers then take the K2 + K6 + K5 path. */
int rls_maxcut_local_search_supported(const rls_graph* g, int64_t B, int32_t num_spin);

/* Which kernel family rls_maxcut_node_cutdeg / rls_maxcut_ls_weights (what = 0) or rls_maxcut_delta_all (what = 1) take for
 * a batch of B envs on this graph: 1 = bit-sliced, lane = node (unweighted graphs; a tile of 64 envs costs the same however
 * few it holds, so from the batch that pays for it), 2 = lane = env tile (weighted graphs, from a larger batch still),
 * 0 = element-parallel.  All three give the same result; tests use this to know which one they exercised. */
int rls_maxcut_node_stats_form(const rls_graph* g, int64_t B, int32_t what);

/* [host] The launch an entry point would make for B envs on this graph: the launchers' own planner, nothing is launched and no
 * pointer of *g is followed (only tested for NULL) -- what tests pin the launch policy with, without a GPU.  `what`: the entry;
 * `flags`: the forms of its arguments (0: byte spins and mask on 16-byte-aligned bases, aligned output, the weights' min / max
 * table present); `cus`: compute units to plan for, <= 0 = the current device's.  Additive (ABI 12). */
enum { RLS_PLAN_K1 = 0, RLS_PLAN_K5 = 1, RLS_PLAN_K6 = 2, RLS_PLAN_K2 = 3, RLS_PLAN_K3 = 4, RLS_PLAN_WEIGHTS = 5 };
enum { RLS_PLAN_F32 = 1, RLS_PLAN_BASE_UNALIGNED = 2, RLS_PLAN_MASK_BITS = 4, RLS_PLAN_OUT_UNALIGNED = 8, RLS_PLAN_NO_MINMAX = 16 };
typedef struct rls_launch_plan {
    int32_t form;   /* 0 / 1 / 2 / 3: bit tiles of 64 / 32 / 16 / 8 envs per workgroup, 4: one env per wave on byte rows, 5 / 6 / 7: K5's
                     * batched / single-wave / generic stream forms, 8: lane = env tile (K2 / K3), 9: element-parallel, 10: refused */
    int32_t waves, planes, vec, wide;   /* template arguments of the kernel: waves per workgroup, counter planes, aligned rows, degrees >= 256 */
    int32_t stage;                      /* the stage argument the kernel receives */
    uint32_t grid, block;               /* workgroups, threads per workgroup */
    int64_t lds;                        /* dynamic LDS bytes */
    int32_t err;                        /* form 10: the code the entry point returns (RLS_EUNSUPPORTED) */
} rls_launch_plan;
int rls_maxcut_launch_plan(const rls_graph* g, int32_t what, int64_t B, int32_t flags, int32_t cus, rls_launch_plan* out);

/* The same local search as separate launches, for graphs rls_maxcut_local_search does not cover (its LDS layout holds
 * two tiles and rd_std: N <= ~7100; these hold one tile: N <= ~15 000 -- and up to N = 39 936 on half tiles of 32 envs
 * (the bare 64-env tile for rows that are not 16-byte multiples, N <= 20 224), through the scratch buffer, which is
 * then REQUIRED; past ~24 900 nodes rd_std is read from global memory and N must be a multiple of 4).  Both use the fused kernel's
 * in-kernel draws -- normal(seed, env_offset + b, node, draw) -- so a caller that passes the same seed gets the result
 * the fused kernel would give.  They replace the torch ops of the decomposed path (randn_like, ws + noise * rd_std,
 * kthvalue, gt: envs/env_L2A.py:95-101, methods/LocalSearch.py:66-72) and K6's mask input.
 *   rls_maxcut_ls_threshold: thresh[b] (f32 [B]) = kthvalue(ws[b,:] + normal(draw) * rd_std, k = N - num_spin)
 *   rls_maxcut_ls_propose:   mask = ws + normal(draw) * rd_std > thresh[b]; rows of x whose x ^ mask has cut >= obj[b]
 *                            take it, obj[b] updated (update_xs_by_vs, util_read_data.py:199)
 * ws / ws_bytes / rd_std as for rls_maxcut_local_search; draw = 0 for the threshold, 1.. for the rounds
 * (0.. when the first draw proposes: LocalSearch.random_search).  ws_pitch = entries between the starts of two rows of ws
 * (0 = N; rls_maxcut_ls_weights writes that layout when given the same pitch): the rows must start 16-byte aligned, which a
 * pitch rounded up to 16 bytes gives for ANY N (the entries between N and the pitch are never read); x may have any N and
 * any alignment. */
int rls_maxcut_ls_threshold(const rls_graph* g, int64_t B, const void* ws, int32_t ws_bytes, int64_t ws_pitch, const float* rd_std,
                            uint64_t seed, int64_t env_offset, int32_t draw, int32_t num_spin, float* thresh, void* scratch,
                            int64_t scratch_bytes, void* stream);
int rls_maxcut_ls_propose(const rls_graph* g, uint8_t* x, int64_t B, const void* ws, int32_t ws_bytes, int64_t ws_pitch,
                          const float* rd_std, const float* thresh, uint64_t seed, int64_t env_offset, int32_t draw, int64_t* obj,
                          void* scratch, int64_t scratch_bytes, void* stream);
/* scratch (16-byte aligned device memory, contents irrelevant, may be shared by all calls of one local search) lets a small
 * batch split each tile's noise pass -- the VALU-bound part -- over up to 8 workgroups: partial top-k lists / bit-packed mask
 * words go through it.  rls_maxcut_ls_scratch_bytes gives the size that enables this for (graph, B, ws_bytes) and num_draws
 * rounds' worth of mask words (1 for the per-round entry points; more than one: every round's, for any batch, while they stay under
 * 1 GiB); 0 = nothing to gain.  With scratch = NULL (or too small) both run one workgroup per tile; the results are the same either way. */
int64_t rls_maxcut_ls_scratch_bytes(const rls_graph* g, int64_t B, int32_t ws_bytes, int32_t num_draws);
/* num_draws rounds of rls_maxcut_ls_propose (draws first_draw, first_draw + 1, ...) in one call.  With scratch of
 * rls_maxcut_ls_scratch_bytes(g, B, ws_bytes, num_draws) bytes a small batch computes the mask words of all rounds first (they do
 * not depend on x) and applies them on ONE load of each tile; otherwise it is the loop over rls_maxcut_ls_propose. */
int rls_maxcut_ls_rounds(const rls_graph* g, uint8_t* x, int64_t B, const void* ws, int32_t ws_bytes, int64_t ws_pitch,
                         const float* rd_std, const float* thresh, uint64_t seed, int64_t env_offset, int32_t first_draw,
                         int32_t num_draws, int64_t* obj, void* scratch, int64_t scratch_bytes, void* stream);
/* The draws of the local-search kernels as a tensor: out f32 [B, N], out[b, n] = normal(seed, env_offset + b, n, draw) -- the
 * value rls_maxcut_local_search / _ls_threshold / _ls_propose use for that (env, node, draw).  Replaces torch.randn_like
 * (envs/env_L2A.py:95,99; methods/LocalSearch.py:66) on the decomposed path (weights wider than 16 bits), so that path too is
 * keyed by the global env id, and feeds the statistical tests of the generator. */
int rls_maxcut_ls_normals(float* out, int64_t B, int64_t N, uint64_t seed, int64_t env_offset, int32_t draw, void* stream);
/* Workgroups per tile the noise passes of a batch of B envs are split over when the scratch buffer is there (1 = the tiles fill the
 * chip by themselves). */
int rls_maxcut_ls_slices(const rls_graph* g, int64_t B, int32_t ws_bytes);
/* 1 when the two entry points above cover this graph / num_spin, else 0 (callers then keep the torch ops + K6). */
int rls_maxcut_ls_rounds_supported(const rls_graph* g, int32_t num_spin);
/* [host] The launches rls_maxcut_local_search / _ls_threshold / _ls_propose / _ls_rounds (`what`) would make, in order: the launchers'
 * own planner (csrc/rls_ls_plan.h), nothing is launched and no pointer of *g is followed -- what tests pin the launch policy with,
 * without a GPU.  ws_pitch in entries (0 = N); `flags`: which buffers are NOT on a 16-byte base, or absent; scratch_bytes as the entry
 * point gets it; `cus`: compute units to plan for, <= 0 = the current device's.  Up to `cap` launches are written to out, info gets
 * their number and, for a refused call, the code and the text the entry point gives (then no launches).  The four host queries above
 * are views of the same planner.  Additive (ABI 12). */
enum { RLS_LS_PLAN_FUSED = 0, RLS_LS_PLAN_THRESHOLD = 1, RLS_LS_PLAN_PROPOSE = 2, RLS_LS_PLAN_ROUNDS = 3 };
enum { RLS_LS_PLAN_X_UNALIGNED = 1, RLS_LS_PLAN_NOISE_UNALIGNED = 2, RLS_LS_PLAN_SCRATCH_UNALIGNED = 4, RLS_LS_PLAN_NO_SCRATCH = 8 };
typedef struct rls_ls_launch {
    int32_t kernel;   /* 0 k_maxcut_local_search<true, WT, planes, waves>, 1 k_ls_threshold<WT, sd_lds>, 2 k_ls_threshold_merge, 3 k_ls_mask<WT, sd_lds>,
                       * 4 k_ls_propose<WT, planes, sd_lds, premask>, 5 k_ls_apply_rounds<planes, waves>, 6 k_ls_apply_rounds32<planes, waves>,
                       * 7 a call of rls_maxcut_propose_accept on the mask words of round `first_round` */
    int32_t ws_bytes, planes, waves, sd_lds, premask;   /* template arguments (WT = int8_t / int16_t by ws_bytes); 0 where the kernel has none */
    uint32_t grid[3], block;
    int64_t lds;                                        /* dynamic LDS bytes */
    int32_t batched, x_aligned, stage, rounds;          /* runtime ints of the kernel: sweep schedule (0), aligned rows (0, 4, 5, 6), has-stage (5, 6),
                                                         * rounds per launch (3: grid[2], 5, 6; 2: the slices it merges) */
    int32_t first_round;                                /* the launch's first draw, counted from the call's */
    int64_t round_words;                                /* 3: words between two rounds' masks */
} rls_ls_launch;
typedef struct rls_ls_plan {
    int32_t err, num_launches;   /* RLS_OK, or what the entry point returns; launches of the whole call (may exceed cap) */
    char msg[288];
} rls_ls_plan;
int rls_maxcut_ls_launch_plan(const rls_graph* g, int32_t what, int64_t B, int32_t ws_bytes, int64_t ws_pitch, int32_t num_spin, int32_t num_draws,
                              int32_t flags, int64_t scratch_bytes, int32_t cus, rls_ls_launch* out, int32_t cap, rls_ls_plan* info);

/* K10 update_xs_by_vs(xs0, vs0, xs1, vs1, if_maximize)  methods/util_read_data.py:190-202:
 *     rows of (xs1, vs1) that are >= (<= when !if_maximize) replace (xs0, vs0). */
int rls_select_better_rows(uint8_t* xs0, int64_t* vs0, const uint8_t* xs1, const int64_t* vs1,
                           int64_t B, int64_t N, int if_maximize, void* stream);

/* K10 pick_xs_by_vs(xs, vs, num_repeats, if_maximize)  methods/util_read_data.py:204-216:
 *     view xs as [R,S,N]; for each s take the r with the best vs (first on ties,
 *     torch.argmax semantics). */
int rls_pick_best_of_repeats(const uint8_t* xs, const int64_t* vs, int64_t R, int64_t S, int64_t N,
                             int if_maximize, uint8_t* good_xs, int64_t* good_vs, void* stream);

/* Evaluator.record2(i, vs, xs)  methods/util_evaluator.py:90-107 without the host read: good = first argmax
 * (argmin when !if_maximize) of vs [B] (vs_kind 0 = int64, 1 = float32, 2 = float64); if good is STRICTLY better
 * than best_v[0] (or force != 0: the constructor's first record), best_v[0] = good and best_x[:] = xs[good, :];
 * improved[0] = 1 | 0; log_v[log_index] = good when log_v != NULL.  best_v double[1], best_x uint8[N], improved
 * uint8[1], log_v double[*]: device memory the host reads only when it prints.  One workgroup. */
int rls_best_update(const uint8_t* xs, const void* vs, int vs_kind, int64_t B, int64_t N, int if_maximize,
                    uint8_t* best_x, double* best_v, uint8_t* improved, double* log_v, int64_t log_index, int force,
                    void* stream);

/* The key of the episode-boundary exchange between ranks ("one int64 key per rank,
 * (best_obj << 20) + (W - 1 - rank)", reduced with MAX = MAXLOC; the single-device analogue is best_vs.argmax(),
 * L2A/demo_instance.py:165) in one launch: key[0] = (max_b vs[b] << rank_bits) | low_code, index[0] (may be NULL) = the first
 * position of the maximum.  vs_kind 0 = int64, 3 = int32, 1 = float32, 2 = float64; float values must be integers or
 * half-integers (the bidirectional envs return count / 2) and are carried doubled.  flag[0] (int32, zeroed by the caller
 * once) gets bit 0 set when |value| >= limit or a float value is not a half-integer: the key is then built from 0. */
int rls_best_key(const void* vs, int vs_kind, int64_t B, int32_t rank_bits, int64_t low_code, int64_t limit, int64_t* key,
                 int64_t* index, int32_t* flag, void* stream);
/* ABI v12.  The reduced key back into what the caller wants, in one launch after the all-reduce (dist.py did it with three
 * [1]-sized torch ops): obj_out = key >> rank_bits as int64[1], or -- as_float -- double[1] = that / 2 (the doubled
 * half-integers of rls_best_key); owner_out (may be NULL) = world - 1 - (key & (2^rank_bits - 1)), the rank whose key won
 * (the `best_vs.argmax()` of L2A/demo_instance.py:165 across ranks).  flag (may be NULL): bit 1 set when key == empty_key,
 * the value a rank without envs contributes -- it survives the MAX only when no rank had any. */
int rls_key_unpack(const int64_t* key, int32_t rank_bits, int64_t world, int as_float, void* obj_out, int64_t* owner_out,
                   int64_t empty_key, int32_t* flag, void* stream);

/* ABI v12.  C2 of the episode-boundary exchange without a host read ("everyone restarts from the best", envs/env_MCPG.py:452-458:
 * best_xs[:] = best_xs[best_vs.argmax()], across ranks).  After the key's all-reduce every rank calls rls_winner_message: the rank
 * whose low code survived in the reduced key[0] writes msg = { (index[0] + env_offset) as 8 little-endian bytes | its row xs[index[0]]
 * bit-packed, bit k of byte j = x[8 j + k] }, every other rank (and a rank with B = 0) zeros -- msg uint8 [8 + ceil(N / 8)].  A
 * SUM all-reduce of msg is then the winner's message on every rank, and rls_winner_unpack turns it into x_out uint8 [N] (may be
 * NULL) and index_out int64[1] (may be NULL).  xs uint8 [B, N] 0|1; B == 1: the row itself (index only supplies the env id).
 * index[0] is read on the device: with B > 1 a value outside [0, B) is "not mine" -- the rank writes zeros, as a rank without envs
 * does -- and never an address outside xs. */
int rls_winner_message(const uint8_t* xs, int64_t B, int64_t N, const int64_t* index, const int64_t* key, int32_t rank_bits,
                       int64_t my_low_code, int64_t env_offset, uint8_t* msg, void* stream);
int rls_winner_unpack(const uint8_t* msg, int64_t N, uint8_t* x_out, int64_t* index_out, void* stream);

/* K14 generate_xs_randomly(num_sims)  envs/env_L2A.py:82-85: i.i.d. Bernoulli(1/2)
 *     spins from a counter-based generator keyed by (seed, global env id), node 0
 *     forced to 0.  env_offset lets a rank generate its shard of a global batch. */
int rls_rand_spins(uint8_t* x, int64_t B, int64_t N, uint64_t seed, int64_t env_offset,
                   void* stream);
/* The same generator for R repeats of S envs in ONE launch (ABI v11): row r * S + s of x [R * S, N] is what
 * rls_rand_spins(seed = repeat_seeds[r], env_offset) writes for env s -- methods/LocalSearch.py:44-50 draws num_sims
 * batches of num_sims random rows in a Python loop.  repeat_seeds: DEVICE uint64 [R]. */
int rls_rand_spins_repeats(uint8_t* x, int64_t R, int64_t S, int64_t N, const uint64_t* repeat_seeds, int64_t env_offset,
                           void* stream);

/* [host] 1 when rls_sub_set_sampling runs S sims x N nodes x R repeats, else 0 (additive: the ABI stays v12).  The limits:
 *   RLS_SUB_SET_SAMPLING_MAX_NODES  a workgroup keeps one sim's determinism row (uint32 [N]), two copies of its start row (N bytes
 *                                   each, rounded up to 16, + 16) and the selected nodes (uint16 [N]) in LDS beside 1040 bytes of
 *                                   scratch: about 8 N <= 160 KB, N <= 20 344 (G70's 10^4 nodes take 81 KB);
 *   1 <= R < 2^31 (the repeat is a 32-bit counter of the generator), 0 <= S < 2^31, top_k >= 0, R S N within int64. */
#define RLS_SUB_SET_SAMPLING_MAX_NODES 20344
int rls_sub_set_sampling_supported(int64_t S, int64_t N, int64_t R, int64_t top_k);

/* sub_set_sampling(probs, start_xs, num_repeats, top_k)  methods/L2A/transformer.py:335-353: the candidates of one policy step
 * (L2A/demo_instance.py:148, demo_distribution.py:160, transformer.py:385) in ONE launch.  Per sim s, with k = min(top_k, N):
 *     det[n] = |probs[s, n] - 0.5|                         one float32 subtraction, exact
 *     selected = the k nodes with the smallest det         (the reference's topk(largest=False); a NaN det orders above every
 *                                                          number, as in torch.topk)
 *     xs_out[r S + s, n] = u(r, s, n) < det[n]  at a selected node, start_xs[s, n] elsewhere        for r = 0 .. R - 1
 *     probs_out[s, n]   = probs[s, n]  at a selected node, (probs[s, n] < 0.5 ? 1 : 0) elsewhere
 * Both quirks are the reference's: the Bernoulli parameter is the determinism, not the probability, and the unselected
 * probabilities come back as 1 below 0.5 and 0 from it on (also for NaN).  Probabilities outside [0, 1] are taken as they are.
 * TIES: where several nodes share the det value at the selection boundary the LOWER node index is selected (torch.topk leaves
 * this unspecified); every NaN counts as the same value.  top_k = 0 copies start_xs R times; top_k >= N selects every node.
 * probs f32 [S, N], start_xs uint8 [S, N] (copied as it is), xs_out uint8 [R S, N] (any byte alignment; written in 16-byte pieces),
 * probs_out f32 [S, N] or NULL; no input is modified and no output may alias an input.
 * uniforms f32 [R S, N] indexed (row, node) -- only the selected entries are read -- or NULL: the counter-based generator of the
 * ISCO steps (murmur3 finaliser, 24 bits to [0, 1)) keyed by (seed, repeat r, env_offset + s, node), so that a rank holding sims
 * [off, off + S_local) of a batch and passing env_offset = off writes exactly its rows (r, s) of the one-process result.
 * The grid is sims x chunks of repeats; every workgroup redoes its sim's selection (a radix select over the N keys in LDS) and
 * patches the row it keeps on chip at the selected nodes only.  RLS_EUNSUPPORTED outside rls_sub_set_sampling_supported, before
 * any launch. */
int rls_sub_set_sampling(const float* probs, const uint8_t* start_xs, int64_t S, int64_t N, int64_t R, int64_t top_k,
                         const float* uniforms, uint64_t seed, int64_t env_offset, uint8_t* xs_out, float* probs_out, void* stream);

/* uniform actions in [0, N) from the same generator (bench / MCMC proposals). */
int rls_rand_actions(int64_t* action, int64_t B, int64_t N, uint64_t seed, uint64_t step,
                     int64_t env_offset, void* stream);

/* ----------------------------------------------------- S2V / ECO / PECO spin system */

/* Resident per-env state of the spin-system env (all device pointers, owned by the caller).  T = float
 * (state_bytes = 4: the batched PECO env, spinsystem_PECO.py) or double (state_bytes = 8: the numpy env,
 * ECO_S2V/src/envs/spinsystem.py). */
typedef struct rls_spin_env {
    void* state;           /* T [B, R, N]: observable rows, row 0 = signed spins {+1,-1} */
    int32_t* delta;        /* [B, N] gain cache: delta[b,i] = s_i * sum_j W_ij s_j ("immediate cuts available",
                            * _get_immeditate_cuts_avaialable, spinsystem_PECO.py:660-661: a dense matmul there) */
    void* score;           /* T [B] */
    void* best_score;      /* T [B] */
    void* best_spins;      /* T [B, N] */
    int32_t* num_nonpos;   /* [B] #{i : delta[b,i] <= 0}, kept incrementally (greedy-actions row, basin test :392-397) */
    int32_t* dist_best;    /* [B] Hamming distance between the spins and best_spins, kept incrementally */
    /* bit-packed spins (needed by the two memories below), or NULL: W = ceil((N + allow_pass) / 64) words per state */
    uint64_t* packed;      /* [B, W] current spins, bit n % 64 of word n / 64 = (s_n > 0) */
    uint64_t* hash;        /* [B] Zobrist hash of packed (pre-filter of the exact compare) */
    /* visited-state memory behind stag_punishment / basin_reward (HistoryBuffer, util_envs_PECO.py:228-288,
     * util_envs.py:355-381), or NULL / 0 */
    uint64_t* hist;        /* [B, hist_cap, W] the state after each earlier step of the episode */
    uint64_t* hist_hash;   /* [B, hist_cap] */
    int64_t hist_cap;
    /* the rows a step changes EVERYWHERE are not stored between observations (a step is O(deg)): */
    int32_t* last_flip;    /* [B, N] the step (1-based) at which the node last flipped in this episode, 0 = not yet */
    void* scalars;         /* T [B, 4] current value of the rows TERMINATION_IMMANENCY, NUMBER_OF_GREEDY_ACTIONS_AVAILABLE,
                            * DISTANCE_FROM_BEST_SCORE, DISTANCE_FROM_BEST_STATE */
    const void* time_table;/* T [table_len]: time_table[k] = 0 + inc + inc + ... (k additions in T, inc = (T)(1 / max_steps)):
                            * what `state[TIME_SINCE_FLIP] += 1. / max_steps` (spinsystem_PECO.py:417) has accumulated after k steps */
    int64_t table_len;     /* >= max_steps + 1 */
    /* options of the single-instance env (spinsystem.py; the batched reference env cannot be constructed with them): */
    void* best_obs_score;  /* T [B] the best OBSERVABLE score: what rewards and the distance rows refer to (= best_score unless
                            * the memory is finite) */
    uint64_t* mem_spins;   /* [B, mem_len, ceil(N / 64)] finite memory (memory_length, spinsystem.py:398-404): the spins after each */
    void* mem_score;       /* T [B, mem_len]             of the last mem_len steps and their scores; NULL / 0 = infinite memory */
    int64_t mem_len;
    int64_t allow_pass;    /* ExtraAction.PASS (spinsystem.py:349-351): action N is legal and flips nothing; the packed spins then
                            * have ceil((N + 1) / 64) words per state, bit N = the parity of the passes (HistoryBuffer,
                            * util_envs.py:361-366, keys its states by the set of actions taken an odd number of times) */
} rls_spin_env;

/* State rows: row 0 (signed spins) and the IMMEDIATE_REWARD_AVAILABLE row of `state` are current after every call; the
 * other observable rows are written by rls_spin_reset, and after steps on demand: rls_spin_observation builds them
 * straight into the observation, rls_spin_materialize writes them into `state`.
 *
 * reset()  spinsystem_PECO.py:150-195 / spinsystem.py:176-252, after the caller has written the signed spins into
 * row 0 of state and their gains into delta (rls_maxcut_delta_all on the spins as bits: the two definitions
 * coincide).  Fills the IMMEDIATE_REWARD_AVAILABLE and NUMBER_OF_GREEDY_ACTIONS_AVAILABLE rows, zeroes the other
 * rows, score = best_score = cut = (weight_sum - sum_i delta_i) / 4 with weight_sum = sum of W over ORDERED pairs,
 * best_spins = spins, num_nonpos, dist_best = 0, last_flip = 0, scalars, packed / hash (the history starts empty: hist_len = 0).
 * row_index [host] int32[7]: as rls_spin_step. */
int rls_spin_reset(const rls_graph* g, const rls_spin_env* env, int state_bytes, int64_t B, int32_t num_rows,
                   const int32_t* row_index, double max_local, int64_t weight_sum, void* stream);

/* One env step of SpinSystemUnbiased  ECO_S2V/src/envs/spinsystem_PECO.py:306-486 (f32, batched) and
 * ECO_S2V/src/envs/spinsystem.py:333-482 (f64, B = 1) on a shared graph: flip action[b]; gain = delta[b,a];
 * incremental update of delta (O(deg), cf. S2V_PPO/env.py:197-206); score += gain; reward (mode 0 DENSE = gain,
 * 1 BLS = max(score - best_before, 0), 2 CUSTOM_BLS = impr / (impr + 0.1), 3 = impr / (impr + 0.05): CUSTOM_BLS for a caller
 * whose score is twice the one kept here -- OptimisationTarget.ENERGY, spinsystem.py:531-543, run as CUT on the negated
 * couplings: -E = 2 cut(-W) + const; with reward_div halved for modes 0 and 1 every reward is the reference's bit for bit), divided by
 * reward_div (n_spins under norm_rewards, else 1); visited-state test against the hist_len earlier states of the episode and append
 * (when env->packed): reward -= stag_punishment on a revisit (use_stag), reward += basin_reward on a first
 * visit of a state with no improving flip (use_basin); best_score / best_spins tracking; last_flip[b, a] = hist_len + 1
 * (hist_len = the number of steps already taken this episode, also without the visited-state memory) and the four
 * scalars.  row_index [host] int32[7] gives the row of IMMEDIATE_REWARD_AVAILABLE,
 * TIME_SINCE_FLIP, EPISODE_TIME, TERMINATION_IMMANENCY, NUMBER_OF_GREEDY_ACTIONS_AVAILABLE,
 * DISTANCE_FROM_BEST_SCORE, DISTANCE_FROM_BEST_STATE in state (-1 = not observed; row 0 is always the signed
 * spins).  reward T [B]; visited_new uint8 [B] or NULL (1 = state not seen before).  The scalar parameters are
 * rounded to T inside (pass the f32-rounded values for the f32 env).  An action outside [0, N) leaves its env
 * untouched and yields reward = NaN.  g->wgt = integer weights or NULL. */
int rls_spin_step(const rls_graph* g, const rls_spin_env* env, int state_bytes, int64_t B, int32_t num_rows,
                  const int32_t* row_index, const int64_t* action, void* reward, uint8_t* visited_new, double max_local,
                  double termination_value, int32_t reward_mode, double reward_div, int64_t hist_len,
                  int32_t use_stag, double stag_punishment, int32_t use_basin, double basin_reward, void* stream);

/* The same env with PER-ENV couplings: the training envs of spinsystem_PECO.py hold matrix T [B, N, N], redrawn by the graph
 * generator at every reset (:150-160; util_envs_PECO.py:40-56, 86-112), and recompute s * (W s) with a batched dense matmul
 * every step.  Here the flipped node's row of its env's matrix is the neighbour list of the same O(changed entries) update.
 *
 * rls_spin_reset_dense: after the caller has written the signed spins into row 0 of state: delta[b,i] = s_i sum_j W_ij s_j,
 * max_local T [B] = max_i sum_j W_ij (_get_immeditate_cuts_avaialable on all-ones spins, :162-168), weight_sum T [B] =
 * sum_ij W_ij, flags uint8 [B]: bit 0 = the reference draws the graph again (sum_i |sum_j W_ij| == 0 or max_local == 0, :164-169),
 * bit 2 = that maximum is 0 although rows with a nonzero (negative) sum exist: max_local then holds the maximum over the NONZERO
 * row sums, which is the rule of the single-instance numpy env (spinsystem.py:190-196: it goes on where the batched env draws again),
 * bit 1 = not a symmetric integer-valued matrix (the int32 gain cache cannot hold it; diagonal entries are allowed and count as
 * in the reference: flipping a changes the score by delta_a - 2 W_aa, :346-348); then everything
 * rls_spin_reset does, with the per-env max_local / weight_sum.  The caller reads flags before stepping. */
int rls_spin_reset_dense(const void* matrix, const rls_spin_env* env, int state_bytes, int64_t B, int64_t N, int32_t num_rows,
                         const int32_t* row_index, void* max_local, void* weight_sum, uint8_t* flags, void* stream);

/* rls_spin_step with matrix T [B, N, N] and max_local T [B] (as rls_spin_reset_dense left them) in place of the shared graph. */
int rls_spin_step_dense(const void* matrix, const void* max_local, const rls_spin_env* env, int state_bytes, int64_t B, int64_t N,
                        int32_t num_rows, const int32_t* row_index, const int64_t* action, void* reward, uint8_t* visited_new,
                        double termination_value, int32_t reward_mode, double reward_div, int64_t hist_len,
                        int32_t use_stag, double stag_punishment, int32_t use_basin, double basin_reward, void* stream);

/* The graph generators of the training envs  ECO_S2V/src/envs/util_envs_PECO.py:15-112 in one launch: matrix T [B, N, N]
 * (state_bytes 4 | 8), symmetric, entries 0 / +-1.
 *   kind 0  RandomERGraphGenerator (:42-57): every pair i < j is an edge with probability p_connection; zero diagonal.
 *   kind 1  RandomBAGraphGenerator (:84-113): seed clique on nodes 0..m INCLUDING its self-loops (as :93-95 sets them), each later
 *           node attached to m_insertion_edges distinct earlier nodes in proportion to their degree (torch.multinomial without
 *           replacement there; uniform draws over the edge-endpoint list with duplicates redrawn here: the same distribution).
 *   edge_type 1 UNIFORM (+1), 2 DISCRETE (one +-1 per node pair, shared by all envs of the call), 3 RANDOM (+-1 per pair and env).
 * Build-defined counter-based draws keyed by (seed, env_offset + b): distributionally equivalent to the reference's torch
 * streams, independent of how the batch is sharded.  N < 65536; kind 1 needs N * m * 6 B of LDS. */
int rls_rand_couplings(void* matrix, int state_bytes, int64_t B, int64_t N, int32_t kind, double p_connection, int32_t m_insertion_edges,
                       int32_t edge_type, uint64_t seed, int64_t env_offset, void* stream);

/* The exact optimum of a spin system by enumeration of all 2^N states: what SpinSystemBase.calculate_best_energy() and its
 * helper _calc_over_range(i0, iMax) of ECO_S2V/src/envs/spinsystem.py:278-324, 615-651 compute (dqn.py:586 and dqn_PECO.py:546
 * call env.calculate_best()[0] for their "distance from optimum" score).  State index i in [0, 2^N) is read MSB first: node k's
 * spin is +1 iff bit N-1-k of i is set (np.binary_repr(i, width=N)).  1 <= N <= 48; couplings symmetric with off-diagonal entries
 * in {-1, 0, +1} and any diagonal (E = -s'Ws / 2 = -tr(W) / 2 + E_off; the trace term is the caller's).
 *
 * rls_spin_exhaustive_pack replaces `matrix = self.matrix.astype('float64')` of _calc_over_range (spinsystem.py:620): matrix T
 * [G, N, N] (state_bytes 4 | 8) -> pos, neg uint64 [G, N]: bit N-1-j of pos[g, p] is set iff W_pj == +1 and j != p, of neg[g, p]
 * iff W_pj == -1 and j != p; flags uint8 [G]: bit 0 = an off-diagonal entry outside {-1, 0, +1}, bit 1 = asymmetric.  All three
 * are results only (written for every graph). */
int rls_spin_exhaustive_pack(const void* matrix, int state_bytes, int64_t G, int64_t N, uint64_t* pos, uint64_t* neg, uint8_t* flags,
                             void* stream);

/* rls_spin_exhaustive replaces the loop of __calc_over_range_jit (spinsystem.py:640-651) over the states i0 <= i < i1
 * (0 <= i0 < i1 <= 2^N): key[g] = min(key[g], ((E_off(i) + 4096) << 48) | i) with E_off = -sum_{p<q} W_pq s_p s_q as int32, one
 * 64-bit atomic minimum per workgroup and graph.  key uint64 [G] is read and written: the caller starts it at INT64_MAX, and
 * chained launches over sub-ranges, or other ranks, fold into the same key -- the lexicographic minimum (lowest energy, then
 * lowest index: the reference's strict `<` in ascending order) does not depend on launch geometry or scheduling.  The maximum of
 * E_off (and so the maximum cut, (sum_{p<q} W_pq + E_off) / 2) is the same call with pos and neg swapped.  The 13-bit field holds
 * every |E_off| <= 2256, the most arbitrary masks can produce at N = 48; masks not made by rls_spin_exhaustive_pack give a
 * meaningless key and never an access outside pos, neg or key.
 * A thread owns aligned chunks of 2^L consecutive indices (L = min(N, 10)): the energy splits into the part among the high N - L
 * nodes (once per chunk, popcounts of masked words), the part among the low L nodes (a table of 2^L entries per workgroup, in
 * reflected Gray order, shared by every chunk) and the cross term, which one add per Gray step keeps current. */
int rls_spin_exhaustive(const uint64_t* pos, const uint64_t* neg, int64_t G, int64_t N, int64_t i0, int64_t i1, uint64_t* key,
                        void* stream);

/* get_observation()  ECO_S2V/src/envs/spinsystem_PECO.py:455,497 (cat(state, matrix_obs)) and spinsystem.py:484-495
 * (vstack(state, matrix)): out T [B, num_rows + N, N] = the num_rows observable rows as the reference's state tensor holds
 * them after step_index steps of the episode (row 0 mapped from signed spins to (1 - s) / 2 when binary_basis,
 * SpinBasis.BINARY; the rows a step does not store built from last_flip / time_table / scalars), followed by the N
 * rows of the matrix: T [N, N] shared by all envs (matrix_per_env = 0) or T [B, N, N] (matrix_per_env = 1); matrix NULL:
 * out = [B, num_rows, N] (the rows only).  One streaming pass, nothing else touched. */
int rls_spin_observation(const rls_spin_env* env, const void* matrix, int32_t matrix_per_env, int state_bytes, int64_t B,
                         int32_t num_rows, int64_t N, const int32_t* row_index, int64_t step_index, int32_t binary_basis, void* out,
                         void* stream);

/* Writes the rows a step does not store (TIME_SINCE_FLIP, EPISODE_TIME, TERMINATION_IMMANENCY, NUMBER_OF_GREEDY_ACTIONS_
 * AVAILABLE, DISTANCE_FROM_BEST_SCORE, DISTANCE_FROM_BEST_STATE) into env->state as the reference holds them after
 * step_index steps: for callers that read the state tensor itself (spinsystem.py's `env.state`). */
int rls_spin_materialize(const rls_spin_env* env, int state_bytes, int64_t B, int64_t N, int32_t num_rows, const int32_t* row_index,
                         int64_t step_index, void* stream);

/* -------------------------------------------------------------------- MCPG */
/* Layouts of a batch of C chains:
 *   spin_bytes = 4 | 1   node-major x[N, C] as in the reference (chains are the fast axis): float32 0.0|1.0 (what
 *                        metro_sampling returns) or uint8;
 *   spin_bytes = 0       bit-packed, tile-major uint64 [ceil(C / 64), N]: word (t, n) holds node n of the chains
 *                        64 t .. 64 t + 63 (bit e = chain 64 t + e; bits of chains >= C are 0).  1/32 of the f32
 *                        surface's bytes, a 64-chain tile is N consecutive words; the form in which a sampling round
 *                        stays on the device (rls_mcpg_pack_chains / rls_mcpg_unpack_chains convert). */

/* [host struct] Global ids of a shard's chains ("per-env RNG keyed by global env id, not rank").  The in-kernel
 * generators of the three entry points below are keyed by (seed, GLOBAL chain id, round / pass / position); the global id of
 * local chain c is
 *     offset + c + (period > 0 ? (c / period) * skip : 0)
 * A rank that owns kept chains [m0, m0 + M_local) of a batch of M kept chains x R repeats (chain = repeat * M + kept, the
 * column order of the reference's  xs_bool.repeat(1, repeat_times), MCPG.py:393-394) passes {m0, M_local, M - M_local}: its
 * chains then draw exactly what they draw in the one-process run, whatever the rank count.  NULL = {0, 0, 0}, the
 * single-process numbering.  period > 0 (with skip > 0) must be a multiple of 64 that divides the launch's chain count C -- the
 * kernels then run one grid row per repeat instead of dividing on the device.  rls_mcpg_local_search_levels draws one coin WORD
 * per 64-chain tile: there offset and skip must be multiples of 64 as well (RLS_EINVAL otherwise).  Recorded draws (index / u /
 * uniforms / coins: test hooks) stay indexed by the LOCAL chain. */
typedef struct rls_chain_ids {
    int64_t offset;
    int64_t period;
    int64_t skip;
} rls_chain_ids;

/* K9  metro_sampling(probs, start_status, max_transfer_time)  methods/MCPG.py:88-117.
 * Runs rounds t = t_offset .. t_offset + min(T, *t_limit_dev) - 1 for every chain c:
 *   i = index[t,c]; p = x[i,c] ? probs[i] : 1 - probs[i];
 *   accept iff u[t,c] < (1 - p) / p  -> flip x[i,c];  accepts[r][t - t_offset] += #accepted chains (r = tile % accept_rows).
 * index int64 [*,C] and u f32 [*,C] are the reference's randint / rand draws in call order (rows
 * indexed by the absolute round t; test mode) or both NULL for the in-kernel counter-based generator
 * (murmur3 finaliser) keyed by (seed, global chain id, t) -- chain_ids [host] maps local chains to global ids (NULL: identity).
 * The reference stops after the first round whose cumulative accept count reaches C*T_transfer
 * samples_in (same dtype, may be NULL = samples) is where the chains are READ; they are written to samples:
 * the first chunk of a call turns the caller's start state into the result buffer without a copy.
 * (one host sync per round there).  Here the caller walks the 5*T_transfer rounds in chunks: a dry
 * call (write_back = 0) fills accepts [accept_rows][T] (int64, zeroed by the caller; a round's count is its COLUMN SUM --
 * workgroups spread their adds over the rows, one row would serialise thousands of atomics per round), the stop round is derived
 * on the device, a second call with t_limit_dev pointing at it (device int64) and write_back = 1
 * applies the chunk; *t_limit_dev <= 0 makes a call return immediately, so chunks after the stop
 * round cost one empty launch.  t_limit_dev NULL = all T rounds.  samples is updated in place only
 * when write_back != 0.
 * C_in (bit-packed layout only; 0 or C otherwise): samples_in holds C_in < C chains, C_in a multiple of 64, and chain c
 * starts from chain c % C_in -- the reference's  xs_bool = temp_max_info.repeat(1, repeat_times)  (MCPG.py:393-394)
 * without materialising the repeat. */
int rls_mcpg_metro_rounds(void* samples, const void* samples_in, int64_t C_in, int spin_bytes, int64_t N, int64_t C,
                          const float* probs, int64_t T, int64_t t_offset, const int64_t* index, const float* u,
                          uint64_t seed, const int64_t* t_limit_dev, int write_back, int64_t* accepts, int64_t accept_rows,
                          const rls_chain_ids* chain_ids, void* scratch, int64_t scratch_bytes, void* stream);
/* ABI v11: `scratch` (device, may be NULL) of at least rls_mcpg_metro_scratch_bytes(N, C) bytes lets the bit-packed walk keep its
 * draw windows (32 KB per 64-chain tile) in L2-resident global memory instead of LDS where that makes room for a second workgroup
 * per CU (N = 10^4: the tile alone is 80 KB); 0 from the query = the windows stay in LDS and scratch is ignored.  Contents are
 * undefined afterwards; results do not depend on it. */
int64_t rls_mcpg_metro_scratch_bytes(int64_t N, int64_t C);

/* The stop rule between two chunks of rls_mcpg_metro_rounds (MCPG.py:103,115: the reference compares `count` with
 * total_mcmc_num * max_transfer_time on the host after every round), one small launch instead of a chain of [T]-sized torch ops:
 * accepts [accept_rows][T] as the chunk's dry (or, for the first chunk, direct) pass filled it; ctl int64 [3] on the device =
 * {accepts of the earlier chunks, walk still live (0 / 1), limit of the next dry pass} -- written, and read unless first != 0;
 * *apply_limit (device int64, may be NULL) = min(this chunk's limit, the first round at which the running count reaches
 * target) for the apply pass; ctl[2] = next_T while the walk is live, else 0 (rls_mcpg_metro_rounds returns at once on 0).
 * first: 1 = the call's first chunk (applied directly: a round accepts at most C proposals, so the count cannot reach C * T
 * before round T), 2 = a later chunk inside the first T rounds, applied directly as well (ctl is read), 0 = a dry pass. */
int rls_mcpg_metro_stop(const int64_t* accepts, int64_t accept_rows, int64_t T, int64_t target, int32_t first, int64_t next_T,
                        int64_t* ctl, int64_t* apply_limit, void* stream);
/* Rounds one rls_mcpg_metro_rounds launch can take with accept counts (the node-major kernels keep them in LDS beside the
 * 64-chain tile: a G81-sized graph, N = 20 000, leaves room for 956); 0 = this layout does not fit at all for N. */
int64_t rls_mcpg_metro_max_rounds(int64_t N, int32_t spin_bytes);

/* K7 + K8 first half  sampler_func  methods/MCPG.py:128-152.
 * xs_in [N,C] holds 0|1 (the sampler's input before the reference maps it to -0.5|1.5).
 * For each of num_ls passes, for pos in 0..N-1, node = order[pos] (int32 [N], degree-descending):
 *     s = sum_{j in nbr(node)} value(j)      value = -0.5|1.5 for nodes not yet visited in
 *                                            pass 0, else 0|1 (MCPG.py:131-133,142)
 *     x[node,c] = (s + u * 0.25f) < (deg(node) + 0.25f) / 2
 * with u = uniforms[pass, pos, c] (f32 [num_ls,N,C], the torch.rand draws in visiting order; NULL =
 * in-kernel Philox / counter hash keyed by (seed, global chain id [chain_ids, host; NULL = identity], pass, position)).  Then expected[c] = sum_e (2x_u - 1)(2x_v - 1) over the stored edge list
 * (= E - 2*cut, exact in f32).  Outputs xs_out f32 [N,C] (0|1) and expected f32 [C].
 * visit_stream (optional, int32) is the visiting order flattened by the caller: visiting positions level-
 * scheduled (a position's level = 1 + max level of its earlier-visited neighbours; sorted by (level, position))
 * and cut into batches of pairwise non-adjacent nodes (<= 32 nodes and <= 400 entries per batch) whose
 * earlier-visited neighbours all sit in earlier batches:
 *     per batch: m, next_batch_offset, 0, off_0 .. off_{m-1}
 *     per node (at stream offset off_k): node, deg, nfresh, visiting position, then deg entries  nb | (fresh << 31)
 * where fresh marks a neighbour visited LATER than node (it still holds -0.5|1.5 in pass 0) and
 * nfresh counts them (rlsolver_amd.methods.MCPG.build_visit_stream builds it).  With it the kernel
 * streams the graph through an LDS ring, the waves of a workgroup share each batch, and nothing waits on
 * global memory per node; NULL selects the generic kernel (one CSR row fetch per node).
 * Weighted graphs (upstream MCPG's weighted MaxCut sampler, methods/MCPG/sampling.py:89-127): edge_weights int32 [E'] in
 * the order of g->eu / g->ev, and a visit stream whose node records are
 *     node, deg, Wfresh, visiting position, Wdeg, then deg PAIRS (nb | fresh << 31, weight)
 * (Wfresh = sum of the weights of the not-yet-visited neighbours, Wdeg = the weighted degree).  The test becomes
 * sum_j w_j v_j + u / 4 < Wdeg / 2 + 0.125 (:114-116) and expected = sum_e w_e (2x_u - 1)(2x_v - 1).  gauge_node >= 0
 * applies that sampler's gauge fix first: every chain is XORed with its own value at gauge_node (:101-104); -1: none.
 * Both need the visit stream (RLS_EUNSUPPORTED without it). */
int rls_mcpg_local_search(const rls_graph* g, const void* xs_in, int spin_bytes, float* xs_out, int64_t C,
                          const int32_t* order, const int32_t* visit_stream, int64_t visit_len, int64_t num_ls,
                          const float* uniforms, uint64_t seed, const int32_t* edge_weights, int64_t gauge_node,
                          float* expected, const rls_chain_ids* chain_ids, void* stream);

/* [host] Level-parallel form of the K7 visiting order (lane = node; same dependency-level argument as
 * rls_graph_sweep_levels, levels taken over visiting POSITIONS: order[pos] = node).  The nodes of a level with degree
 * <= 128 are packed into groups of 64 LANES, sorted by degree; a row too long for the level's cap (chosen per level by
 * an instruction-count estimate: none / 32 / 16 / 8 entries per lane, always <= 64) takes L = 2, 4 or 8 ADJACENT lanes,
 * lane j of them holding neighbours j, j + L, ... -- the kernel adds the lanes' counters before the compare, so a
 * level's longest row costs deg / L rounds and pads 63 lanes that much less.  A node of higher degree forms a group of
 * its own and is decided with lane = neighbour.  Group record in lv_data (ABI v11: LANE-major, so that a lane fetches its
 * header in one 8-byte load and a block of 8 rounds in two 16-byte loads):
 *     64 x 2 words  per lane l, words 2 l and 2 l + 1:
 *                   node | K << 20 | log2 L << 28 | tie << 31   K = ceil(deg / 2), tie = deg even               (passes >= 1)
 *                   pos  | K0 << 20 | tie0 << 31      K0 = ceil((deg + nfresh) / 2), tie0 = (deg + nfresh) even  (pass 0)
 *     per block of 8 rounds, 2 slabs of [64 lanes][4 rounds]: round r of lane l at 128 + 512 (r / 8) + 256 ((r / 4) % 2) + 4 l + r % 4:
 *                   8 nb | fresh << 31      (8 nb = byte offset of the neighbour's word in the tile); padding: 8 N
 * (rounds = the longest lane's, rounded up to a multiple of 8; idle lanes carry node = N; a hub group uses lane 0's two header
 * words -- K / K0 in 11 bits, no L --, word 4 = deg, and lists neighbour r in round r / 64 of lane r % 64).  Behind the last
 * record come sixteen spare rows (a group's header and first two blocks are requested unguarded), and behind those THE SAME TABLE
 * AGAIN with the fresh flags cleared, at offset (lv_ptr[groups] & 0x3fffffff) + 1024: passes >= 1 read it and use an entry as
 * the LDS address it is.  *total counts both copies.
 * The accept rule of MCPG.py:139-141, (s + u/4) < (deg + 1/4)/2 with s in half-integers, is  2s < deg, or
 * 2s == deg and u < 1/2 (in float32: see methods/MCPG.py tie_coins_from_uniforms):
 * new bit = [count < K] | ([count == K] & tie & coin), count = #ones among the neighbours
 * (pass 0: #ones among visited + 2 #ones among not-yet-visited ones, against K0).
 * lv_ptr [host, groups+1]: offset | bit 31 = first group of a level | bit 30 = hub group.  NULL outputs: sizing.
 * Needs N < 2^20 and max degree < 1024. */
int rls_mcpg_visit_levels(const int32_t* rowptr, const int32_t* col, int64_t N, const int32_t* order, int32_t* lv_ptr,
                          int64_t ptr_capacity, int32_t* lv_data, int64_t data_capacity, int64_t* num_groups,
                          int64_t* total);

/* K7 + K8 first half on that schedule (production path: tie coins from a counter hash keyed by (seed, GLOBAL 64-chain
 * block [chain_ids, host; NULL = identity], pass, position); coins uint64 [num_ls * N, ceil(C / 64)] -- bit c % 64 of word [pass * N + pos, c / 64] =
 * "u < 1/2" for chain c -- replaces them for tests).  Same outputs as rls_mcpg_local_search; xs_out is float32
 * node-major (out_spin_bytes = 4) or bit-packed (0; then xs_out may alias a bit-packed xs_in).  C_in: as in
 * rls_mcpg_metro_rounds.  The caller's contract, like a tour: lv_data holds the `total` entries that lv_ptr's offsets name -- the
 * entry point is told num_groups, not that length, and does not check it. */
int rls_mcpg_local_search_levels(const rls_graph* g, const void* xs_in, int spin_bytes, int64_t C_in, void* xs_out,
                                 int out_spin_bytes, int64_t C, const int32_t* lv_ptr, const int32_t* lv_data,
                                 int64_t num_groups, int64_t num_ls, const uint64_t* coins, uint64_t seed, float* expected,
                                 const rls_chain_ids* chain_ids, void* stream);

/* 1 when rls_mcpg_local_search_levels covers this graph with a schedule of num_groups groups (bit tile + group
 * offsets + scratch within 160 KB of LDS, unweighted, N < 2^20, degrees < 1024), else 0. */
int rls_mcpg_local_search_levels_supported(const rls_graph* g, int64_t num_groups);

/* K8 second half  methods/MCPG.py:154-161: best_index[m] = m + M * argmin_r expected[r*M + m]
 * (first minimum), vs_good[m] = (num_edges - expected[best]) / 2, xs_good[:, m] = xs[:, best].
 * M = total_mcmc_num, R = repeat_times, xs f32 [N, M*R], xs_good f32 [N, M]. */
int rls_mcpg_pick_best(const float* expected, const void* xs, int spin_bytes, int64_t N, int64_t total_mcmc_num,
                       int64_t repeat_times, int64_t num_edges, int64_t* best_index, float* vs_good,
                       void* xs_good, void* stream);

/* The best-merge of the MCPG outer loop  methods/MCPG.py:376-391 on bit-packed kept chains (M = total_mcmc_num,
 * temp_info / now_info uint64 [ceil(M/64), N]), all on the device:
 *   for m: if temp_max[m] > now_max_res[m]: now_max_res[m] = temp_max[m]; now_info[:, m] = temp_info[:, m]   (:377-380)
 *   hi = first argmax, lo = first argmin of now_max_res; now_max_res[lo] = now_max_res[hi];
 *   now_info[:, lo] = now_info[:, hi]; temp_info[:, lo] = now_info[:, hi]                                     (:383-391)
 * temp_info afterwards is the start state of the next round (rls_mcpg_metro_rounds with C_in = M).  mask_scratch
 * uint64 [ceil(M/64)]; best_value f32 [1] / best_index int64 [1] (may be NULL) receive max(now_max_res) and its chain.
 * replace_worst = 0 (a rank's shard of the kept chains: the worst and the best incumbent are properties of the WHOLE batch):
 * only the per-chain merge (:377-380) is applied, and best_value / best_index are [2] = {max, min} of the shard's now_max_res
 * and their first chains -- what the caller needs to replace the global worst by the global best itself. */
int rls_mcpg_merge_best(const float* temp_max, uint64_t* temp_info, float* now_max_res, uint64_t* now_info, int64_t N,
                        int64_t total_mcmc_num, uint64_t* mask_scratch, float* best_value, int64_t* best_index,
                        int32_t replace_worst, void* stream);

/* What get_return  methods/MCPG.py:292-302 needs from the samples: A[n] += sum_c value[c] * s[n, c] over the C
 * bit-packed chains (A f32 [N], zeroed by the caller).  With s in {0,1},  log(s p + (1-s)(1-p)) summed over nodes is
 * sum_n log(1-p_n) + sum_n s_n (log p_n - log(1-p_n)), so the objective mean_c(log_prob_sum_c * value_c) and its
 * gradient with respect to p follow from A and sum(value) -- the [C, N] float products are never formed. */
int rls_mcpg_value_bit_sums(const uint64_t* samples, int64_t N, int64_t C, const float* value, float* A, void* stream);

/* node-major uint8 / float32 [N, C] -> bit-packed tiles, and back to float32 (the shims of the reference-shaped API) */
int rls_mcpg_pack_chains(const void* xs, int spin_bytes, int64_t N, int64_t C, uint64_t* packed, void* stream);
int rls_mcpg_unpack_chains(const uint64_t* packed, int64_t N, int64_t C, float* xs, void* stream);

/* K11 mcpg_sampling_qubo / mcpg_sampling_qubo_bin  methods/MCPG/sampling.py:323-370 (after the
 * metro step): num_ls Gauss-Seidel sweeps  x_i <- [Q[i,:] . x (x_i := 0) > thr_i]  over variables in
 * index order, then value[c] = x^T Q x.  binary = 0: spins +-1, thr = 0 (:332-340); binary = 1:
 * spins 0|1, thr = -Q_ii / 2 (:357-365).  Q f32 [n,n] dense; xs_in/xs_out f32 [n,C] node-major holding
 * 0|1 (the +-1 variant maps 0 -> -1 internally and returns (s+1)/2 as the reference does).
 * Exact for integer-valued Q (f32 sums order-independent below 2^24). */
int rls_qubo_local_search_value(const float* Q, int64_t n, const float* xs_in, float* xs_out, int64_t C,
                                int64_t num_ls, int binary, float* value, void* stream);

/* K11, sparse form: the same coordinate search and value with Q in CSR form -- rowptr int32
 * [n+1], col int32 [nnz], val f32 [nnz], the diagonal stored as ordinary entries; step i costs O(nnz_i), not O(n).
 * Same arguments and outputs otherwise; same exactness condition (integer-valued Q).
 * ABI v12: lv_ptr int32 [num_levels + 1] / lv_rows int32 [n] (both NULL = none): the rows grouped by level(i) = 1 + max level of
 * the neighbours j < i (rows in ascending order within a level) -- rows of one level share no entry, so the waves of a
 * workgroup sweep them side by side and the result is the sequential sweep's; without them one wave walks the rows in order. */
int rls_qubo_sparse_local_search_value(const int32_t* rowptr, const int32_t* col, const float* val, int64_t n,
                                       const int32_t* lv_ptr, const int32_t* lv_rows, int32_t num_levels,
                                       const float* xs_in, float* xs_out, int64_t C, int64_t num_ls, int binary,
                                       float* value, void* stream);

/* [host] 1 when the K11 call of this form runs n variables x C chains within its LDS budget, else 0 (the call would return
 * RLS_EUNSUPPORTED; an addition that changes no existing entry, so the ABI stays v12).  form 0: rls_qubo_local_search_value
 * (dense); 1: rls_qubo_sparse_local_search_value without a level schedule; 2: with one (the level kernel, or the sequential
 * kernel where the level kernel's LDS does not fit).  Both kernels accept any square Q -- symmetric or not, empty rows,
 * nnz = 0 -- the sparse one with a level schedule built over the symmetrised pattern (Q_ij != 0 or Q_ji != 0). */
int rls_qubo_local_search_supported(int64_t n, int64_t C, int32_t form);

/* K12 mcpg_sampling_mimo  methods/MCPG/sampling.py:296-313 (after the metro step): the MIMO detection sampler's coordinate
 * search and value on K11's block scheme (additive: the ABI stays v12).  Sigma f32 [n, n] dense (any square matrix: the diagonal
 * is NOT masked, the reference's loaders zero it), Diag f32 [n].  Chains bit-packed tile-major uint64 [ceil(C / 64), n] (bit 1 =
 * +, bit 0 = -); xs_in may hold C_in < C chains, C_in a multiple of 64: chain c reads chain c % C_in (C_in <= 0 = C); xs_out may
 * be xs_in when C_in == C; bits of chains past C leave as 0.
 *   info = +-2 (every variable, before its first visit);  num_ls sweeps over i = 0 .. n-1:
 *     r = Sigma[i, :] . info  (the current info, info_i included);  info_i = +1 if r < -Diag_i / 2 else -1  (strict: a tie is -1)
 *   expected[c] = sum_i info_i (Sigma info)_i + Diag . info      (to be MINIMISED; the reference returns -(min + sca)).
 * f32 in, f32 accumulate on the matrix cores; sums run in another order than the reference's matmul.  Bit-exact with it for
 * integer-valued Sigma / Diag when  2 sum_j |Sigma_ij| + |Diag_i| < 2^24  for every row i and  sum |Sigma| + sum |Diag| < 2^24.
 * num_ls < 1 is RLS_EINVAL (+-2 entries would survive).  xs_out == NULL: no sweep, nothing written but expected of the chains
 * as +-1 (num_ls is not read).  n beyond the LDS budget (rls_mimo_local_search_supported) is RLS_EUNSUPPORTED. */
int rls_mimo_local_search(const float* Sigma, const float* Diag, int64_t n, const uint64_t* xs_in, int64_t C_in, uint64_t* xs_out,
                          int64_t C, int64_t num_ls, float* expected, void* stream);

/* [host] 1 when rls_mimo_local_search runs n >= 1 variables x C chains within its LDS budget (K11's: n <= 30 720 / 35 840 /
 * 15 872 by form), else 0.  *form (may be NULL) = the launch form this shape gets, chosen by K11's rule from C and the CU count:
 * 0 = 32-chain workgroups of 8 waves, 1 = 32-chain workgroups of 4 waves, 2 = 64-chain workgroups of 4 waves. */
int rls_mimo_local_search_supported(int64_t n, int64_t C, int32_t* form);

/* ------------------------------------------------------------------ MaxSAT */

/* [host] Level schedule of mcpg_sampling_maxsat's sweep  methods/MCPG/sampling.py:259-271 (additive: the ABI stays v12).
 * The formula is a clause CSR: clause_ptr int32 [M + 1], lit int32 [L] signed +-(v + 1), weight int32 [M] (>= 1) or NULL = all
 * ones; order int32 [nvar] = the visiting order (ndata[3]).  For variable i the reference lists, once per OCCURRENCE of i, the
 * whole clause the occurrence sits in (dataloader.py:240-247: a clause that holds i twice is listed twice) and keeps the flip
 * where  sum_listed max_lit(s_v neg)  grows, a uniform draw deciding only ties (new - old is an even integer).  A listed clause
 * moves that sum by +-2w when no literal of ANOTHER variable satisfies it and i's own literals in it have one sign; so with
 * crit = ~OR_others (x_v ^ sign), make = weight of the critical clauses whose own literal is false, break = of those whose own
 * literal is true, the rule is  x_i ^= [make > break] | ([make == break] & coin).
 * level(position) = 1 + the highest level of an earlier-visited variable that shares a clause with it: the variables of a level
 * share no clause, so deciding level after level from the pre-level state is the sequential sweep.  Positions are sorted by
 * (level, stream length descending) and cut into groups of 64 LANES, lane = variable.
 * lv_ptr [host, groups + 1]: (record offset / 64) | planes << 24 | weighted << 30 | first group of a level << 31; planes = counter
 * planes the group's largest listed weight sum needs (1 .. 24).  Group record in lv_data:
 *     64 x 2 words   lane l: variable (nvar on idle lanes), visiting position (keys the coin)
 *     per block of 4 rounds, [64 lanes][4 rounds] (a lane fetches a block in one 16-byte load), round r of lane l at
 *     128 + B (r / 4) + 4 l + r % 4, B = 256:   8 v | sign << 31 | ends << 0 | class << 1
 *         = one literal of another variable of the listed clause (8 v = byte offset of its word in the LDS tile; sign = negated);
 *           `ends` marks the clause's last entry and carries the variable's own sign class in it (1 positive, 2 negative, 3 both:
 *           the clause cannot change).  A clause without other literals, and one of class 3, is the single entry 8 nvar | ends |
 *           class (word nvar of the tile is zero); so is padding (8 nvar, ends = 0).
 *     weighted (weight != NULL): B = 512 and the block's second half holds the weights, that of a clause beside its last entry.
 * The table ends in 512 spare words (a lane requests its next block unguarded).  NULL outputs: sizing (*num_groups, *total).
 * A stream is never split over lanes: a variable of 600 clauses costs its group 600+ rounds.
 * Limits (rls_maxsat_local_search_supported): nvar <= 20 445 (8 bytes per variable and the zero word + 272 bytes of tables in 160 KB of LDS); the
 * sum of all clause weights, and of the weights listed for one variable, below 2^24 (the reference's own exact float32 range):
 * RLS_EUNSUPPORTED beyond.  A literal 0 or past nvar, a weight < 1, an order that is no permutation: RLS_EINVAL. */
int rls_maxsat_visit_levels(const int32_t* clause_ptr, const int32_t* lit, const int32_t* weight, int64_t nvar, int64_t M,
                            const int32_t* order, int32_t* lv_ptr, int64_t ptr_capacity, int32_t* lv_data, int64_t data_capacity,
                            int64_t* num_groups, int64_t* total);

/* [host] 1 when the MaxSAT sampler covers nvar variables and clause weights that sum to weight_sum, else 0; the limits themselves
 * go to *max_nvar / *max_weight_sum (largest accepted values; either may be NULL). */
int rls_maxsat_local_search_supported(int64_t nvar, int64_t weight_sum, int64_t* max_nvar, int64_t* max_weight_sum);

/* The sweep and the score of mcpg_sampling_maxsat  methods/MCPG/sampling.py:257-274 in ONE kernel, one workgroup per 64-chain
 * tile, the tile uint64 [nvar] in LDS, every operation 64 chains wide in one lane, make / break in bit-sliced counters.
 * xs_in: bit-packed chains holding 0|1 (the sampler maps them to -1|+1), C_in as in rls_mcpg_metro_rounds; xs_out: bit-packed
 * (out_spin_bytes = 0; may alias xs_in when C_in == C) or float32 node-major [nvar, C] (4).  num_ls passes over the schedule of
 * rls_maxsat_visit_levels (lv_ptr / lv_data on the device); num_ls = 0: the pure scorer.  Tie coins: counter hash keyed by
 * (seed, GLOBAL 64-chain block [chain_ids, as rls_mcpg_local_search_levels], pass, position), or coins uint64
 * [num_ls * nvar, ceil(C / 64)] -- bit c % 64 of word [pass * nvar + pos, c / 64] = "u < 1/2" for chain c (tests).
 * Then expected[c] = -S[c], S = sum over the clauses of the CSR (device: clause_ptr [M + 1], lit, weight or NULL) of
 * max_lit(s_v neg) = +w for a satisfied clause, -w for an unsatisfied one, 0 for an empty one (:272-274).  The reference's
 * res = (S + K) / 2 is rls_mcpg_pick_best's (num_edges - expected) / 2 with num_edges := K, its first argmax of res that
 * kernel's first argmin of expected: K never enters this launch.  lit must not be NULL when M > 0, also where every clause is
 * empty (it is then never read). 
 * The caller's contract, like a tour: lv_data holds the `total` entries of rls_maxsat_visit_levels and lit the clause_ptr[M]
 * literals -- the entry point is told num_groups and M, not those lengths, and does not check them. */
int rls_maxsat_local_search(const void* xs_in, int64_t C_in, void* xs_out, int out_spin_bytes, int64_t C, int64_t nvar,
                            const int32_t* lv_ptr, const int32_t* lv_data, int64_t num_groups, int64_t num_ls,
                            const uint64_t* coins, uint64_t seed, const int32_t* clause_ptr, const int32_t* lit,
                            const int32_t* weight, int64_t M, float* expected, const rls_chain_ids* chain_ids, void* stream);

/* ------------------------------------------------------------ Cheeger cuts */

/* [host] 1 when the Cheeger sampler covers a graph of N nodes and E stored edges whose weights sum to weight_abs_sum in absolute
 * value, else 0 (additive: the ABI stays v12).  The two limits:
 *   RLS_CHEEGER_MAX_NODES  the 64-chain tile uint64 [N] is all the kernel keeps in LDS: N <= 160 KB / 8 = 20 480 (*max_N, may be NULL);
 *   RLS_CHEEGER_EXACT      weight_abs_sum + 2 E < 2^24 and N < 2^24: cut, size and every intermediate of the rule below are then
 *                          integers or half-integers that float32 holds exactly, as they are in the reference. */
#define RLS_CHEEGER_MAX_NODES 20480
#define RLS_CHEEGER_EXACT (1 << 24)
int rls_cheeger_local_search_supported(int64_t N, int64_t E, int64_t weight_abs_sum, int64_t* max_N);

/* The sweep and the score of mcpg_sampling_rcheegercut / mcpg_sampling_ncheegercut  methods/MCPG/sampling.py:181-250 in ONE
 * kernel: lane = chain, one wave per 64-chain tile, the tile uint64 [N] in LDS, cut / size / h in registers.  Per chain, float32:
 *     s_v = 2 x_v - 1;  cut = (edge_weight_sum - sum_e s_u s_v) / 2   (the edge sum is UNWEIGHTED, over g's stored edges: :190-191)
 *     size = sum_v x_v;  h = cut / min(size, N - size)  (normalized = 0, :193)   |   cut * (1 / size + 1 / (N - size))  (1, :229)
 *     num_ls times, for every node in visiting order:
 *         c = sum_{j in neighbours[node]} x_j              unweighted, with multiplicity (a self-loop lists the node twice)
 *         ncut = cut - s_node (weighted_degree[node] - 2 c);  nsize = size - s_node;  nh = the same formula on (ncut, nsize)
 *         keep = (h < nh) or (min(nsize, N - nsize) < 1e-7);  if not keep: flip x_node and cut, size, h = ncut, nsize, nh
 * The rule draws nothing and is sequential per chain: every decision reads cut, size and h as the flips before it left them.
 * Divisions are IEEE (1 / 0 = inf, 0 / 0 = NaN, 0 * inf = NaN); NaN exists only before the first visit (num_ls = 0).
 * xs_in: bit-packed chains holding 0|1, C_in as in rls_mcpg_metro_rounds; xs_out: bit-packed (out_spin_bytes = 0; may alias
 * xs_in when C_in == C) or float32 node-major [N, C] (4).  visit_stream int32 [3 N + nnz] on the device, one record per visiting
 * position:  node, degree, weighted degree, then the `degree` neighbours (node = index of its uint64 word in the tile); a record
 * that points past N or past stream_len ends the pass.  num_ls = 0 only scores.  Outputs f32 [C]: h, and cut / size after the
 * last pass (either may be NULL).  RLS_EUNSUPPORTED outside rls_cheeger_local_search_supported (|edge_weight_sum| stands in for
 * the absolute sum, which a caller checks on the host); RLS_EINVAL for a stream of another length. */
int rls_cheeger_local_search(const rls_graph* g, const void* xs_in, int64_t C_in, void* xs_out, int out_spin_bytes, int64_t C,
                             const int32_t* visit_stream, int64_t stream_len, int normalized, int64_t num_ls, float edge_weight_sum,
                             float* h, float* cut, float* size, void* stream);

/* ------------------------------------------------------- edge-flip MaxCut */

/* [host] 1 when the edge-flip MaxCut sampler covers a graph of N nodes and E stored edges whose largest sum of |weights| at a node
 * is max_abs_degree, whose |weights| sum to weight_abs_sum and whose visit stream holds stream_len words, else 0 (additive: the ABI
 * stays v12).  The limits:
 *   RLS_MAXCUT_EDGE_MAX_NODES  the 64-chain tile uint64 [N] and a bitmap of the written nodes (N bits) are what the kernel keeps in
 *                              LDS: 8 N (rounded up to 16) + 4 ceil(N / 32) <= 160 KB, N <= 20 164 (*max_N, may be NULL);
 *   RLS_MAXCUT_EDGE_EXACT      3 max_abs_degree < 2^24 (a neighbour sum t is a half-integer of at most 1.5 max_abs_degree: the
 *                              kernel counts 2 t in integers, and float32 holds it exactly, as it does in the reference) and
 *                              weight_abs_sum < 2^24 (the score is an integer float32 holds exactly);
 *   stream_len < 2^31. */
#define RLS_MAXCUT_EDGE_MAX_NODES 20164
#define RLS_MAXCUT_EDGE_EXACT (1 << 24)
int rls_maxcut_edge_local_search_supported(int64_t N, int64_t E, int64_t max_abs_degree, int64_t weight_abs_sum, int64_t stream_len,
                                           int64_t* max_N);

/* Everything after the walk of mcpg_sampling_maxcut_edge  methods/MCPG/sampling.py:141-172 in ONE kernel (the loader's per-edge
 * rows and `add` table, methods/MCPG/dataloader.py:87-101, :125-153, arrive as the visit stream): lane = chain, one wave per
 * 64-chain tile, the tile uint64 [N] in LDS.  Per chain:
 *     gauge_node >= 0: x ^= x[gauge_node] (:142-144); a node then holds v = 2 x - 0.5 until its first write, x afterwards (:145)
 *     num_ls times, for every position i of the stream (edge e = sorted_degree_edges[i], r = eu[e], c = ev[e]):
 *         t_r = sum_k w_k v[nbr_k] over row(r) less its first entry c, t_c over row(c) less its first entry r   (:161-162)
 *         a = (t_r + u0 * 0.1f) + add0;  b = (t_c + u1 * 0.1f) + add1;  z = ((a + b) + u2 * 0.1f) - add2     (float32, :163-165)
 *         k = first maximum of (z, a, b, 0);  x[r] = k >> 1, then x[c] = k & 1                                  (:166-168)
 *     expected = sum_e edge_weights[e] (2 x_u - 1)(2 x_v - 1) over g's stored edges                             (:172)
 * The sweep is sequential per chain.  num_ls = 0 applies the gauge and scores.
 * xs_in: bit-packed chains holding 0|1, C_in as in rls_mcpg_metro_rounds; xs_out: bit-packed (out_spin_bytes = 0; may alias
 * xs_in when C_in == C; a node never written holds its gauge-fixed bit) or float32 node-major [N, C] (4; a node never written
 * holds -0.5 | 1.5, as in the reference).  edge_weights int32 [E'] in the order of g's stored edges.  visit_stream int32
 * [stream_len] on the device (methods/MCPG.py: build_edge_stream), one record per position:
 *     r, c, len_r, len_c, add0, add1, add2 (float32 bits), then len_r + len_c pairs (nbr | fresh << 31, weight)
 * fresh = the neighbour has not been an endpoint of an earlier position; it is read in pass 0 only.  A record that points past N
 * or past stream_len ends the pass; neighbour indices are clamped into the tile.
 * uniforms f32 [num_ls, E', 3, C]: u0, u1, u2 per (pass, position) in the reference's draw order, or NULL: the counter generator
 * (murmur3 finaliser) keyed by (seed, global chain id -- chain_ids [host], NULL = identity --, pass, position, which of the
 * three), 24 bits to [0, 1).  expected f32 [C].  Chains past C write nothing.
 * RLS_EUNSUPPORTED outside rls_maxcut_edge_local_search_supported (max_abs_degree and weight_abs_sum are the caller's host-side
 * figures); RLS_EINVAL for a stream shorter than 7 E' or a gauge_node that is neither a node nor -1. */
int rls_maxcut_edge_local_search(const rls_graph* g, const int32_t* edge_weights, const void* xs_in, int64_t C_in, void* xs_out,
                                 int out_spin_bytes, int64_t C, const int32_t* visit_stream, int64_t stream_len, int64_t max_abs_degree,
                                 int64_t weight_abs_sum, int gauge_node, int64_t num_ls, const float* uniforms, uint64_t seed,
                                 float* expected, const rls_chain_ids* chain_ids, void* stream);

/* --------------------------------------------------------------------- TSP */

/* K12 ISCO_TSP.calculate_distance(sample)  envs/env_ISCO.py:346-350.
 * len[b] = sum_k D[p[k], p[k+1]] + D[p[N-1], p[0]], f32, sequential k order. */
int rls_tsp_tour_length(const float* dist, int64_t N, const int64_t* perm, int64_t B,
                        float* length, void* stream);

/* K13 ISCO_TSP.opt_2(sample, temperature)  envs/env_ISCO.py:238-335 (ABI v12: the whole of it).
 * For every position i of every tour: the partner CITY (:245-262: rand < K / (K + 1) ? nearest[city_i, randint(K)] :
 * random[city_i, randint(N - K - 1)]), j = its position in perm[b] (:265-272), ban = the partner is a neighbour of position
 * i + 1 (:291-293), delta of swapping the cities at positions i + 1 and j (:318-333).  Outputs logratio = -delta /
 * temperature f32 [B,N], indices int64 [B,N], ban uint8 [B,N].
 *   selected == NULL (production): the partners are drawn IN the kernel from (seed, env_offset + b, i) -- the generator and the
 *     counters of rls_isco_tsp_step's iteration 0 -- through nearest int32 [N, K] / random int32 [N, random_stride]
 *     (random_stride >= N - K - 1; or their byte form tables8, below), near_threshold = K / (K + 1); selected_out (may be
 *     NULL) records them, int64 [B,N].  1 <= K <= N - 2 (RLS_EINVAL otherwise): the far draw needs a non-empty table, as the
 *     reference's randint(0, N - K - 1) does.
 *     Algorithmic bytes per tour: 8N in, 13N out.
 *   selected != NULL (the recorded-draw hook of the golden tests): int64 [B,N] partner cities, tables / seed ignored. */
int rls_tsp_swap_delta_all(const float* dist, int64_t N, const int64_t* perm, int64_t B, const int64_t* selected,
                           const int32_t* nearest, int32_t K, const int32_t* random, int32_t random_stride, const uint8_t* tables8,
                           float near_threshold, uint64_t seed, int64_t env_offset, int64_t* selected_out, float temperature,
                           float* logratio, int64_t* indices, uint8_t* ban, void* stream);
/* tables8 (may be NULL; N <= 256): the same two tables as BYTES for the kernel to keep in LDS beside the distance matrix --
 * rls_tsp_tables8_bytes(N, K) bytes, 4-byte aligned: uint8 [N, K] nearest, zero-padded to a multiple of 16 bytes, then uint8
 * [N, N - K - 1] = the first N - K - 1 columns of random, zero-padded likewise (0 = no byte form for this N / K: N > 256, or K outside [1, N - 2]). */
int64_t rls_tsp_tables8_bytes(int64_t N, int32_t K);

/* [host] The form a TSP entry point takes at these sizes: the launchers' own arithmetic (csrc/rls_tsp_plan.h -- they call the
 * same functions), nothing is launched and no device is needed; what tests assert the form they mean to reach with.
 *   what = RLS_TSP_TOUR_LENGTH (K12), RLS_TSP_SWAP_DELTA (K13: K and has_tables8 describe the in-kernel draw -- has_tables8 = 1:
 *   selected == NULL and the caller passes tables8; 0: tables8 == NULL or recorded `selected`, K ignored), RLS_TSP_STEP
 *   (rls_isco_tsp_step), RLS_TSP_2OPT_BEST / _EXACT (cur_length == NULL / given), RLS_TSP_RAND_PERMS.  K and has_tables8 are
 *   read for RLS_TSP_SWAP_DELTA only.
 * Fills *out; returns RLS_EINVAL for N < 1, an unknown `what` or out == NULL.  A size the entry point refuses is NOT an error
 * here: supported = 0 (the entry point returns RLS_EUNSUPPORTED before any launch), the other fields 0.
 * Additive (the ABI stays v12). */
enum { RLS_TSP_TOUR_LENGTH = 0, RLS_TSP_SWAP_DELTA = 1, RLS_TSP_STEP = 2, RLS_TSP_2OPT_BEST = 3, RLS_TSP_RAND_PERMS = 4,
       RLS_TSP_2OPT_BEST_EXACT = 5 };
enum { RLS_TSP_KERNEL_ONLY = 0, RLS_TSP_KERNEL_PERMS_LDS = 1, RLS_TSP_KERNEL_PERMS_GLOBAL = 2 };
typedef struct rls_tsp_form {
    int32_t lds_d;      /* 1: the distance matrix is staged in LDS (the LDS_D = true instantiation) */
    int32_t tab8;       /* 1: K13 keeps the byte tables in LDS (TAB8 = true; implies lds_d) */
    int32_t block;      /* threads per workgroup */
    int32_t waves;      /* waves per workgroup (K12 / K13 / the step: tours in flight per workgroup) */
    int64_t lds_bytes;  /* dynamic LDS bytes of the launch */
    int32_t kernel;     /* RLS_TSP_KERNEL_*: which of rls_rand_perms' two kernels; RLS_TSP_KERNEL_ONLY elsewhere */
    int32_t supported;  /* 0: the entry point returns RLS_EUNSUPPORTED at this size */
} rls_tsp_form;
int rls_tsp_launch_form(int32_t what, int64_t N, int32_t K, int32_t has_tables8, rls_tsp_form* out);

/* ISCO_TSP.switch  envs/env_ISCO.py:337-344 for one chosen position per env:
 * if pos[b] >= 0 swap perm[b, (pos[b]+1) % N] and perm[b, indices[b, pos[b]]]. */
int rls_tsp_apply_swap(int64_t* perm, int64_t B, int64_t N, const int64_t* pos,
                       const int64_t* indices, void* stream);

/* true 2-opt (segment reversal) delta for a closed tour, the move of
 * methods_problem_specific/TSP/opt_2.py:27-57: reversing perm[i..j] changes
 * the length by D[p[i-1],p[j]] + D[p[i],p[j+1]] - D[p[i-1],p[i]] - D[p[j],p[j+1]].
 * i, j int64 [B] with 0 <= i <= j < N. */
int rls_tsp_2opt_delta(const float* dist, int64_t N, const int64_t* perm, int64_t B,
                       const int64_t* i, const int64_t* j, float* delta, void* stream);

/* One pass of local_search_2_opt  methods_problem_specific/TSP/opt_2.py:27-57: over all reversals [i..j], 0 <= i < j <= N-1,
 * of the closed tour perm[b] (evaluated against that same tour, as the reference restores its seed after every candidate)
 * the best one, the first in (i, j) order among equals.  dist float64 [N, N].
 *   cur_length != NULL (float64 [B], the length the reference holds for the seed): candidates are compared by their WHOLE
 *     length summed the way distance_calc does (float64, edge after edge) -- the reference's own comparison values, so
 *     reversals that tie in exact arithmetic rank as they do there.  best_value[b] = that length (< cur_length[b]) and
 *     (best_i, best_j)[b] the pair, or cur_length[b] and (-1, -1) when no candidate is shorter.  O(N) per candidate.
 *   cur_length == NULL: candidates are compared by delta(i, j) = D[a,c] + D[b,e] - D[a,b] - D[c,e] (rls_tsp_2opt_delta's
 *     formula in float64; SYMMETRIC dist), O(1) per candidate: best_value[b] = the most negative delta, or 0 / (-1, -1).
 * perm rows must be permutations of 0..N-1 (not checked on the device).
 * slices >= 1 workgroups share the candidates of one tour (a lone tour still fills the chip): best_i, best_j and best_value
 * must then hold slices * B entries; the results are the first B of each (the rest is scratch). */
int rls_tsp_2opt_best(const double* dist, int64_t N, const int64_t* perm, int64_t B, const double* cur_length, int32_t slices,
                      int64_t* best_i, int64_t* best_j, double* best_value, void* stream);

/* One pass of local_search_3_opt  methods_problem_specific/TSP/opt_3.py:42-105 (segments_3_opt :27-37, distance_calc :17-22).
 * The reference's move reverses blocks in place and moves none: for every triple (i, j, k), 0 <= i < j < N, j < k < N + (i > 0),
 * in that order, the open tour perm[b] is cut into H = p[0..i], S1 = p[i+1..j], S2 = p[j+1..min(k, N-1)], C = the rest (S2 and C
 * may be empty), and seven trials are evaluated against that same tour, numbered in the reference's order
 *     0 aBC   1 AbC   2 ABc   3 Abc   4 abC   5 aBc   6 abc        (a lower-case letter: S1 / S2 / C reversed).
 * The result is the first strict minimum in (i, j, k, trial) order; trials that reproduce the seed tour are evaluated too.
 * dist float64 [N, N], N >= 3; perm int64 [B, N] open 0-based tours (permutations of 0..N-1: not checked on the device).
 *   cur_length != NULL (float64 [B], the length the reference holds for the seed): a candidate's value is the length of its
 *     closed tour summed as distance_calc does (float64, edge after edge from position 0, the closing edge last) -- the
 *     reference's own comparison values, for any matrix.  best_value[b] = the winner's length (< cur_length[b]), or
 *     cur_length[b] with (best_i, best_j, best_k, best_trial)[b] = -1 when no candidate is strictly shorter.
 *   cur_length == NULL (SYMMETRIC dist): only the junctions between consecutive non-empty blocks change, in cyclic order H|S1,
 *     S1|S2, S2|C, C|p[0] (an empty block is skipped).  With x_q / y_q the new / old edge of junction q = 1..m, m <= 4:
 *     value = (((x_1 + x_2) + x_3) + x_4) - (((y_1 + y_2) + y_3) + y_4) in float64, each sum left to right, compared with 0.
 *     best_value[b] = the most negative value, or 0 with -1 indices.
 * slices in [1, 65535] workgroups share one tour's candidates: the five outputs must then hold slices * B entries each; the
 * results are the first B of each (the rest is scratch: rows of [slices, B] partial results).
 * RLS_EUNSUPPORTED where the tour no longer fits LDS (rls_tsp_3opt_launch_form).  Additive (the ABI stays v12). */
int rls_tsp_3opt_best(const double* dist, int64_t N, const int64_t* perm, int64_t B, const double* cur_length, int32_t slices,
                      int64_t* best_i, int64_t* best_j, int64_t* best_k, int64_t* best_trial, double* best_value, void* stream);

/* [host] The form rls_tsp_3opt_best takes at N (exact = 1: cur_length given): the launcher's own arithmetic (csrc/rls_tsp3_plan.h),
 * nothing is launched.  Fills lds_d (the float64 matrix is staged in LDS), block, waves, lds_bytes = lds_d * 8 N^2 + exact * 8 (N + 1)
 * + 16 waves + 4 N, kernel = RLS_TSP_KERNEL_ONLY, tab8 = 0; supported = 0 (other fields 0) where the entry point returns
 * RLS_EUNSUPPORTED.  RLS_EINVAL for N < 3 or out == NULL. */
int rls_tsp_3opt_launch_form(int64_t N, int32_t exact, rls_tsp_form* out);

/* The order in which the constructors of methods_problem_specific/TSP take up cities: nn.py:62-75 (nearest_neighbour),
 * ins_n.py:84-96 (nearest_insertion), ins_f.py:84-96 (farthest_insertion, farthest = 1).  chain[s, 0] = start[s] and chain[s, k + 1]
 * = the city c not yet in the chain with the smallest (farthest = 1: largest) dist[chain[s, k], c]; among equal values the lowest
 * city index (numpy's first extremum -- the reference masks visited rows, columns and the diagonal with +-inf, which leaves exactly
 * these cities).  dist float64 [N, N] with finite entries, N >= 2; start int64 [S]; chain int64 [S, N]; status int32 [S]: 0, or 2
 * where start[s] lies outside [0, N) -- that row of chain is then left as it was and nothing is read out of bounds.
 * One wave per start, N sequential steps.  RLS_EUNSUPPORTED for N > 163840 (a byte per city in LDS).  Additive (the ABI stays v12). */
int rls_tsp_neighbour_chain(const double* dist, int64_t N, const int64_t* start, int64_t S, int32_t farthest, int64_t* chain,
                            int32_t* status, void* stream);

/* Grow-and-converge: the inner work of nearest_insertion / farthest_insertion / cheapest_insertion (best_insertion ins_n.py:61-68,
 * ins_c.py:61-84) and of nearest_neighbour's local search (nn.py:80-81), one persistent workgroup per row, one launch.
 * For row s the open tour starts as order[s, 0:m_seed]; then for m = m_seed .. m_end:
 *     if m > m_seed, order[s, m - 1] is appended at the end of the tour;
 *     if m >= first_m, best-improvement 2-opt passes of opt_2.py:27-57 run on the closed m-city tour until a pass finds nothing
 *     strictly shorter than the tour's length -- a pass is rls_tsp_2opt_best with cur_length given, bit for bit: every reversal
 *     [i..j], 0 <= i < j <= m - 1, valued by distance_calc's sequential float64 sum from the candidate's first city, the first
 *     strict minimum in (i, j) order kept.
 * dist float64 [N, N] (N is the matrix stride, m the tour length); order int64 [S, N]; 2 <= m_seed <= m_end <= N; first_m any
 * (> m_end: no pass at all); max_passes >= 1.
 *   tours int64 [S, N]: tours[s, :m_end] the tour, tours[s, m_end:] = order[s, m_end:] (a permutation stays one);
 *   length float64 [S]: the sequential float64 sum of the closed tour from tours[s, 0], the closing edge last;
 *   passes int64 [S]: evaluated passes, the fruitless one that ends each convergence included;
 *   status int32 [S]: 0; 1: a convergence reached max_passes improving passes -- the row holds the state after that pass (the
 *     cities appended so far, the rest of order behind them) and grows no further.  The loop ends by itself, lengths strictly
 *     decrease: max_passes only guarantees that the kernel returns; 2: an entry of order[s] lies outside [0, N): tours, length and
 *     passes of the row are left as they were.  Repeated cities in a row are not detected (they index inside dist).
 * The matrix is staged in LDS while it fits (rls_tsp_grow_launch_form); RLS_EUNSUPPORTED where even the tour no longer does.
 * Additive (the ABI stays v12). */
int rls_tsp_grow_2opt(const double* dist, int64_t N, const int64_t* order, int64_t S, int64_t m_seed, int64_t m_end, int64_t first_m,
                      int64_t max_passes, int64_t* tours, double* length, int64_t* passes, int32_t* status, void* stream);

/* [host] The form rls_tsp_grow_2opt takes at N: the launcher's own arithmetic (csrc/rls_tsp_grow_plan.h), nothing is launched.
 * Fills lds_d (the float64 matrix is staged in LDS: N <= 141), block = 1024, waves = 16, lds_bytes = lds_d * 8 N^2 + 8 (N + 1)
 * + 16 waves + 8 N, kernel = RLS_TSP_KERNEL_ONLY, tab8 = 0; supported = 0 (other fields 0) where the entry point returns
 * RLS_EUNSUPPORTED (N >= 10224).  RLS_EINVAL for N < 2 or out == NULL. */
int rls_tsp_grow_launch_form(int64_t N, rls_tsp_form* out);

/* ------------------------------------------------------------------- ISCO sampler steps */

/* ISCO_maxcut.step(x, path_length, temperature)  envs/env_ISCO.py:26-49 in ONE kernel (one wave per env):
 *   ll_x = cut(x) / T;  log_prob = log_softmax(gain / 2T)   (get_local_dist :51-63: the closed form of the autograd)
 *   Gumbel top-k without replacement of path_length[b] nodes  (multinomial, methods/util.py:514-555) -> mask, ll_x2y
 *   y = x with the masked nodes flipped; ll_y, log_prob(y); ll_y2x = probability of undoing the selection in
 *   reverse order (ll_y2x :65-77);  log_acc = min(ll_y + ll_y2x - ll_x - ll_x2y, 0);
 *   y_out[b] = accepted ? y : x  with  log(u_accept + 1e-24) < log_acc   (mh_step, methods/util.py:556-570)
 * x, y_out f32 [B, N] holding 0|1 (y_out may alias x); path_length int64 [B], clamped to [1, N] as the caller's
 * torch.clamp does (methods/ISCO/main_ISCO_maxcut.py:26).  u_gumbel f32 [B, N] and u_accept f32 [B]: the
 * reference's two torch.rand draws in call order (tests), or both NULL: counter-based generator keyed by
 * (seed, env_offset + b, node).  Outputs (each may be NULL): energy_out f32 [B] = ll_y * T (of the PROPOSAL, as
 * the reference returns it), acc_out f32 [B] = exp(log_acc), terms_out f32 [B, 5] = ll_x, ll_x2y, ll_y, ll_y2x,
 * log_acc, mask_out uint8 [B, N] = the selected nodes.  Unweighted (the reference's energy ignores weights).
 * scratch: device memory of rls_isco_maxcut_scratch_bytes(g, B) bytes -- 0 (scratch may be NULL) while a sample's rows fit LDS
 * (N <= ~15 900); past that the two f32 rows of every sample (log-probabilities, perturbed values: 8 N bytes) live there and a
 * workgroup takes each sample (N <= ~81 000: the two byte rows still sit in LDS; RLS_EUNSUPPORTED beyond).  Contents need not
 * survive between calls. */
int64_t rls_isco_maxcut_scratch_bytes(const rls_graph* g, int64_t B);
int rls_isco_maxcut_step(const rls_graph* g, const float* x, float* y_out, int64_t B, const int64_t* path_length,
                         float temperature, const float* u_gumbel, const float* u_accept, uint64_t seed,
                         int64_t env_offset, float* energy_out, float* acc_out, float* terms_out, uint8_t* mask_out,
                         void* scratch, int64_t scratch_bytes, void* stream);

/* ISCO_MIS.step(x, path_length, temperature)  envs/env_ISCO.py:111-174 in ONE kernel: rls_isco_maxcut_step with the energy of
 * the maximum-independent-set sampler (model :162-170) in place of the cut,
 *   ll_x = (sum_i x_i - lam * pairs(x)) / T,  pairs = edge-list entries (u, v) with x_u = x_v = 1: a duplicated line counts
 *          twice, a loop (u, u) once when u is set;
 *   log_prob = log_softmax((1 - 2 x_i) (1 - lam * cnt_i) / 2T),  cnt_i = set neighbours of i over its row entries (a loop is
 *          listed twice in its row)  -- the closed form of get_local_dist's autograd (:134-146).
 * Everything else is rls_isco_maxcut_step's contract, word for word: x / y_out / path_length (clamped to [1, N]) / the two
 * draws (both given or both NULL: the same generator and key layout, (seed, env_offset + b, node)) / the outputs and the
 * terms_out layout / y_out must not alias x / RLS_EUNSUPPORTED past the byte rows' limit.  lam (the reference's LAMADA = 1.001)
 * must be finite.  g as ISCO_maxcut builds it: one row entry per end of every edge-list line, loops kept.
 * scratch: rls_isco_maxcut_scratch_bytes(g, B) -- the rows and their layout are the same. */
int rls_isco_mis_step(const rls_graph* g, const float* x, float* y_out, int64_t B, const int64_t* path_length,
                      float temperature, float lam, const float* u_gumbel, const float* u_accept, uint64_t seed,
                      int64_t env_offset, float* energy_out, float* acc_out, float* terms_out, uint8_t* mask_out,
                      void* scratch, int64_t scratch_bytes, void* stream);

/* PISCO_maxcut.tensor_core_energy's product  envs/env_ISCO.py:436-444 (XA = matmul(delta_x, adj_matrix), :439) on the f16 matrix
 * instruction (f16 operands, f32 accumulate):  r_out f32 [B, Np] = delta(x) . A,  delta_k = x_k > 0 ? +1 : -1.
 * adj = A, IEEE binary16 [Np, Np] row-major (the reference's adj_matrix: zero-padded from n to Np = ceil(n / 8) * 8 nodes,
 * methods/ISCO/util_maxcut.py:17-35); x binary16 [B, Np]; both 16-byte aligned, Np a positive multiple of 8.  Padded columns of
 * x count (x = 0 is delta = -1): the zero rows of A silence them.  A need not be symmetric here.  The result is not rounded to
 * f16; it is exact while every |sum| stays below 2^24 on integer-valued A. */
int rls_pisco_product(const uint16_t* adj, int64_t Np, const uint16_t* x, int64_t B, float* r_out, void* stream);

/* Bytes of scratch rls_pisco_step needs: r f32 [B, Np] followed by ord int32 [B, Np] = 8 B Np (0 for B <= 0 or an Np that is no
 * positive multiple of 8).  Host query, nothing is launched. */
int64_t rls_pisco_scratch_bytes(int64_t Np, int64_t B);

/* PISCO_maxcut.step(x, path_length, temperature)  envs/env_ISCO.py:384-434 (get_local_dist :407-416, tensor_core_energy :436-444,
 * proposal :394-405, ll_y2x :418-430; multinomial methods/ISCO/util.py:19-60): rls_pisco_product, then ONE kernel that is
 * rls_isco_maxcut_step with the local distribution of a sample read from its row of r:
 *   ll_x = -0.25 * sum_k r_k delta_k / T;  log_prob = log_softmax(delta_k r_k / 2T) over all Np columns (a padded column scores 0
 *   and can be selected and flipped, as in the reference);
 *   the proposal's row is r'_j = r_j - 2 sum_{k selected} delta_k A[k][j] -- A must be SYMMETRIC (the closed-form gradient and
 *   this update both assume it; the reference builds A from an undirected graph).
 * half_rounding != 0 (the reference's arithmetic): r, r' and sum_k r_k delta_k are each rounded to binary16 once before use;
 * 0: everything stays f32.  x, y_out binary16 [B, Np] holding 0|1 (x > 0 reads as 1); y_out must not alias x.  path_length,
 * temperature, the two draws (both or neither; generator keyed by (seed, env_offset + b, column)), energy_out / acc_out /
 * terms_out / mask_out (uint8 [B, Np]): as rls_isco_maxcut_step.  scratch: rls_pisco_scratch_bytes(Np, B) bytes, 16-byte aligned,
 * clobbered.  Checks, all before the first launch and in this order: Np % 8, B (0 is a no-op), temperature > 0, Np past the
 * rows-in-LDS limit (~16 000 columns: RLS_EUNSUPPORTED with the byte counts; there is no rows-in-scratch form), then the pointers,
 * aliasing and scratch_bytes.  RLS_ISCO_FORCE_WG / RLS_ISCO_SEL_CAP act as for the other steps. */
int rls_pisco_step(const uint16_t* adj, int64_t Np, const uint16_t* x, uint16_t* y_out, int64_t B, const int64_t* path_length,
                   float temperature, int32_t half_rounding, const float* u_gumbel, const float* u_accept, uint64_t seed,
                   int64_t env_offset, float* energy_out, float* acc_out, float* terms_out, uint8_t* mask_out, void* scratch,
                   int64_t scratch_bytes, void* stream);

/* [host] The launch rls_isco_maxcut_step / rls_isco_mis_step (dense = 0) or rls_pisco_step (dense != 0, N = Np) make for B samples
 * of N nodes on a device of `cus` compute units, under the tuning knobs as they stand (csrc/rls_isco_plan.h; no device needed):
 * out[0] wg (1: a workgroup per sample, 0: a wave per sample), out[1] grows (1: the two f32 rows in the caller's scratch),
 * out[2] P and out[3] Pw (capacity of the selected-set list of the workgroup / the wave form; a larger selection is ordered by
 * extraction), out[4] waves (samples per workgroup of the wave form), out[5] lds (dynamic LDS bytes of the chosen form),
 * out[6] err (RLS_OK, or the code the step returns without launching), out[7] need (LDS bytes of the smallest form: what a
 * refusal reports).  Returns RLS_OK whenever it answers -- a refusal of the step is out[6], not the return value. */
int rls_isco_launch_plan(int64_t N, int64_t B, int cus, int dense, int64_t* out);

/* ISCO_TSP.step(x, path_length, temperature)  envs/env_ISCO.py:188-236 in ONE kernel (one wave per env, the tour,
 * its inverse and -- when it fits -- the distance matrix in LDS): path_length times { opt_2 (:238-335: partner
 * city per position from the nearest / random tables, swap delta, ban mask) -> logits = -delta / 2T (banned:
 * -5e5) -> log_softmax -> one Gumbel draw -> selected position q; ll_x2y = log_prob[q]; ll_y2x = log_softmax of
 * the logits with entry q negated, at q (y2x :214-226); swap positions q + 1 and j(q) unless banned (switch
 * :337-344) }, then log_acc = min(sum of the delta_yx, -ll_x2y, ll_y2x terms, 0) and the Metropolis accept
 * between perm_in and the walked tour.  nearest int32 [N, K], random int32 [N, random_stride] of which columns 0 .. N-K-2 are drawn from (the
 * reference's table has N - 1 columns, ISCO/util_TSP.py:9-16),
 * near_threshold = (float)(K / (K + 1)) as the reference's comparison sees it.  Test draws, all or none:
 * u_partner f32, r_near int64, r_rand int64, u_gumbel f32, each [path_length, B, N] in call order, u_accept f32
 * [B].  perm_out int64 [B, N] (must not alias perm_in); log_acc_out / acc_out f32 [B] and cur_out int64 [B, N]
 * (the walked tour before the accept) may be NULL. */
int rls_isco_tsp_step(const float* dist, int64_t N, const int32_t* nearest, int32_t K, float near_threshold,
                      const int32_t* random, int32_t random_stride, const int64_t* perm_in, int64_t* perm_out, int64_t B, int32_t path_length,
                      float temperature, const float* u_partner, const int64_t* r_near, const int64_t* r_rand,
                      const float* u_gumbel, const float* u_accept, uint64_t seed, int64_t env_offset,
                      float* log_acc_out, float* acc_out, int64_t* cur_out, void* stream);

/* The row moves of evolutionary_replacement  methods/util.py:87-94:  xs[dst[k]] = xs[src[k]], vs[dst[k]] =
 * vs[src[k]] for k < K (dst and src disjoint: top_ids vs low_ids there).  xs uint8 [*, N], vs int64 or NULL. */
int rls_copy_rows(uint8_t* xs, int64_t* vs, int64_t N, const int64_t* dst, const int64_t* src, int64_t K, void* stream);
/* The same moves with the row count (additive: the ABI stays v12).  dst and src are read on the device: a move with dst[k] or
 * src[k] outside [0, B) is skipped -- xs, vs and everything around them stay as they were -- where rls_copy_rows, which is not
 * told B, can only skip a negative index.  xs uint8 [B, N], vs int64 [B] or NULL.  Call this one. */
int rls_copy_rows_bounded(uint8_t* xs, int64_t* vs, int64_t B, int64_t N, const int64_t* dst, const int64_t* src, int64_t K, void* stream);

/* ---- The MaxCut env of S2V_PPO  methods/S2V_PPO/env.py: a batch of envs on DIFFERENT graphs (additive: the ABI stays v12).
 * The batch is laid out like a torch_geometric Batch: env i owns nodes [ptr[i], ptr[i + 1]) of every per-node array, and ONE CSR by
 * source over all nodes holds the edge-list entries as given (env.py:199 reads rows edge_index[0] == a and nothing else: a line
 * listed twice counts twice, a loop (u, u) is an ordinary entry, a one-directional line stays one-directional); each row is sorted
 * by destination (stable), columns are global node ids inside the row's own env.  All pointers are device memory; the struct lives
 * on the host.  No scratch is needed. */
typedef struct rls_s2vppo_env {
    int64_t num_envs, total_nodes, max_nodes;   /* B, sum of N_i (< 2^31), the largest N_i (chooses the launch form) */
    int64_t nnz, tenure, multiplier;            /* entries; config.tabu_tenure >= 0; config.episode_length_multiplier >= 1 */
    const int64_t* ptr;        /* [B + 1] */
    const int64_t* rowptr;     /* [total_nodes + 1] */
    const int32_t* col;        /* [nnz] */
    const float* w;            /* [nnz] */
    const float* wtot;         /* [B, 3]: W = sum(w) / 2 (env.py:19), W + 1e-8 as float32 (env.py:119), and 1 when the graph's list equals
                                * its transpose, weights included (the greedy reset then updates gains in O(deg) per flip), else 0 */
    int8_t* z;                 /* [total_nodes] -1 | +1 */
    float* delta;              /* [total_nodes] delta_cache: z_i * sum of w z_dst over i's row */
    int32_t* last_flip;        /* [total_nodes] step count at the node's last flip: time_since_flip = step_count - last_flip */
    int8_t* best_z;            /* [total_nodes] */
    int32_t* counters;         /* [B, 4]: step_count, recorded basins, episodes begun, source of the start spins (0 z0, 1 random, 2 greedy) */
    double* cut;               /* [B] current_cut (also the step's info['cut_value']) */
    double* best_cut;          /* [B] */
    int32_t* tabu;             /* [B, max(tenure, 1)] ring of the last `tenure` actions, slot (step - 1) % tenure */
    int64_t* hash;             /* [B, 51]: ring of the last 50 state hashes (slot step % 50) and the current one */
    int64_t* basins;           /* [multiplier * total_nodes]: env i records at most max_steps_i basins from multiplier * ptr[i] */
    float* x;                  /* [total_nodes, 5] node features, rewritten in place (env.py:116-131) */
    uint8_t* mask;             /* [total_nodes] valid_actions_mask (env.py:107-114) */
} rls_s2vppo_env;

/* [host] The launch rls_s2vppo_step / _reset make for B envs whose largest graph has max_nodes nodes (csrc/rls_s2vppo_plan.h):
 * out[0] form (0: a wave per env, 1: a workgroup per env), out[1] threads per workgroup, out[2] envs per workgroup, out[3] workgroups. */
int rls_s2vppo_launch_plan(int64_t B, int64_t max_nodes, int64_t* out);

/* EnvMaxcut.step  S2V_PPO/env.py:140-206 for every env of the batch in ONE launch (train_ddp.py:117-139 loops over env objects).
 * action int64 [B], LOCAL node ids.  Per env, in the reference's order: cut += delta[a] (:141-144); z[a] = -z[a]; delta[dst] +=
 * 2 z[dst] z[a] w over a's row, entries of one destination added in list order by one lane (:197-205; a loop sees the new z[a]); THEN
 * delta[a] = -delta[a] (:206); step_count, the tabu ring, last_flip (:150-156); `new` = the state's hash is not among the last 50
 * (:159-160); reward in float64 (:163-183): (cut - best) / ((cut - best) + 0.1) if the cut beats the best (best_cut, best_z follow),
 * - stag_punishment if not new, + 0.01 if every delta <= 0 and the hash is no recorded basin (it is then recorded); THEN the hash
 * joins the history (:186); done = step_count >= multiplier * N (:188); x and mask are rewritten (:107-131).
 * A state's identity is a 64-bit Zobrist hash (XOR of a fixed key(local node) over the nodes with z = +1); the reference compares
 * Python hashes of the spin bytes.  Two different states of one episode collide with probability about 2^-64 per pair.
 * reward f64 [B], done uint8 [B].  An action outside [0, N_i) leaves its env untouched and reports reward = NaN, as rls_maxcut_step
 * does (the reference raises an IndexError); so does an env whose step_count has reached multiplier * N (done stays 1): the basin
 * table holds one episode, reset it first.  No host read, no allocation: capturable in a HIP graph.
 * The action's row is walked in strides of the group, but a run of equal destinations is added by ONE thread in list order: a row
 * costs its longest run, not d / threads. */
int rls_s2vppo_step(const rls_s2vppo_env* e, const int64_t* action, double stag_punishment, double* reward, uint8_t* done, void* stream);

/* EnvMaxcut.reset  S2V_PPO/env.py:46-74 for the envs ids[0 .. num_ids) (distinct), or for all of them (ids NULL, num_ids = B), in ONE
 * launch.  The start spins: z0 int8 [total_nodes] when given (test hook: only the listed envs' nodes are read); else greedy uint8 [B]
 * when given chooses per env (1: from all-ones flip the node with the largest gain, ties to the lowest index, while that gain is > 0,
 * at most N / 2 times :51-57 -- the gains follow a flip through the node's row when the list is its own transpose, else all are recomputed; 0: independent +-1 spins :49); else a coin decides.  Coin and spins come from the counter-based generator
 * of the ISCO steps keyed by (seed, env_offset + env, the env's episode counter, node).  Then delta, cut = W / 2 - sum(z nb) / 4, best =
 * cut, best_z = z, the hash; counters and rings start over; x and mask are written. */
int rls_s2vppo_reset(const rls_s2vppo_env* e, const int64_t* ids, int64_t num_ids, const int8_t* z0, const uint8_t* greedy, uint64_t seed,
                     int64_t env_offset, void* stream);

/* B random permutations (random_gen_init_sample, env_ISCO.py:352-354). */
int rls_rand_perms(int64_t* perm, int64_t B, int64_t N, uint64_t seed, int64_t env_offset,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RLSOLVER_HIP_H */
