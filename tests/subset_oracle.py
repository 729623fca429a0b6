"""numpy restatement of sub_set_sampling (rlsolver/methods/L2A/transformer.py:335-353) with the draws as an input and the
package's tie rule: where several nodes share the determinism at the selection boundary, the LOWER node index is selected
(torch.topk leaves that unspecified; every golden row has distinct values there).  Not the reference's code: the rule, restated."""
import numpy as np

NAN_KEY = np.uint32(0x7FC00000)      # every NaN determinism is one key, above +inf (torch.topk orders NaN as the largest value)


def determinism(probs):
    """(det f32 [S, N] = |probs - 0.5| in float32, its ordering key uint32 [S, N])."""
    det = np.abs(np.asarray(probs, dtype=np.float32) - np.float32(0.5))
    key = det.view(np.uint32).copy()
    key[np.isnan(det)] = NAN_KEY
    return det, key


def selected_mask(probs, top_k):
    """bool [S, N]: the min(top_k, N) nodes of each sim with the smallest determinism, ties to the lower node index."""
    det, key = determinism(probs)
    S, N = det.shape
    k = min(int(top_k), N)
    order = (key.astype(np.uint64) << np.uint64(32)) | np.arange(N, dtype=np.uint64)[None, :]     # distinct: (det, node)
    idx = np.argsort(order, axis=1, kind="stable")[:, :k]
    sel = np.zeros((S, N), dtype=bool)
    np.put_along_axis(sel, idx, True, axis=1)
    return sel


def boundary_is_distinct(probs, top_k):
    """The condition every golden row meets: its k-th and (k+1)-th smallest determinism differ (or there is no boundary)."""
    _, key = determinism(probs)
    N = key.shape[1]
    k = min(int(top_k), N)
    if k == 0 or k == N:
        return True
    sk = np.sort(key, axis=1)
    return bool(np.all(sk[:, k - 1] != sk[:, k]))


def sub_set_sampling(probs, start_xs, num_repeats, top_k, uniforms):
    """-> (xs bool [R S, N], probs f32 [S, N]).  uniforms f32 [R S, N] indexed (row r S + s, node): only selected entries are read."""
    probs = np.asarray(probs, dtype=np.float32)
    start = np.asarray(start_xs).astype(bool)
    R = int(num_repeats)
    det, _ = determinism(probs)
    sel = selected_mask(probs, top_k)
    xs = np.tile(start, (R, 1))
    sel_r, det_r = np.tile(sel, (R, 1)), np.tile(det, (R, 1))
    with np.errstate(invalid="ignore"):
        drawn = np.asarray(uniforms, dtype=np.float32) < det_r          # (u < NaN is False, as in torch)
        probs_out = np.where(sel, probs, (probs < np.float32(0.5)).astype(np.float32))
    xs[sel_r] = drawn[sel_r]
    return xs, probs_out.astype(np.float32)
