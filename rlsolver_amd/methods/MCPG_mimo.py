"""MIMO detection family of the upstream MCPG package -- drop-in for rlsolver/methods/MCPG/sampling.py:288-320
(mcpg_sampling_mimo), dataloader.py:297-396 (read_data_mimo3, read_data_mimo5) and the driver's table and epilogue
(MCPG.py:108-171, :184-193), on HIP tensors.

    metro_sampling -> info = (x - 1/2) 4 = +-2 -> num_ls sweeps over the variables in index order,
    info_i = +1 if Sigma[i] . info < -Diag_i / 2 else -1 (the CURRENT info, info_i included; a tie gives -1)
    -> expected = info^T Sigma info + Diag . info -> the FIRST minimum over the repeats of each kept chain
    -> (-(expected[best] + sca), (info + 1) / 2 of the best, the walk's output, expected - mean(expected)).

The walk is the package's metro walk (methods/MCPG.py); everything between it and the best of repeats is ONE kernel
(include/rlsolver_hip.h: rls_mimo_local_search, K11's block Gauss-Seidel on the matrix cores over bit-packed chains).  A variable
holds +-2 until its first visit, so at least one sweep is required: num_ls < 1 is refused.

The reference's loaders leave Sigma / Diag in float64 and its sampler multiplies them with float32 chains, which torch refuses: it
runs only with the data cast to float32.  Here the loaders compute in float64 as the reference does and cast at the end; Sigma / Diag
are float32 on the device.  No data file ships with the reference: mimo_instance generates instances, write_mimo3 / write_mimo5
write the two file forms.

For MCPGRound / run_mcpg a Data_MIMO stands where a MaxCut graph stands (see the class)."""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch

from .. import ops_mcpg_tsp as mops
from ..ops_mcpg_tsp import PackedChains
from .MCPG import metro_sampling
from .MCPG_maxcut_edge import value_of

TEN = torch.Tensor


class Data_MIMO(list):
    """[Sigma f32 [n, n], Diag f32 [n], X f64 [n] (the sent symbols, +-1), sca f64 0-dim, noise float] -- data[0] .. data[4] as the
    reference's loaders return them, Sigma / Diag cast to float32 -- + ``num_nodes`` and ``device``.

    For MCPGRound / run_mcpg the object stands where a MaxCut graph stands: ``round_local_search`` hands back 2 expected,
    ``num_edges`` is 0 and ``value_scale`` 0.5, so that the round's best-of-repeats value (num_edges - 2 expected) / 2 is -expected
    (its incumbents are maximised) and its value expected - mean(expected), both exactly (doubling commutes with float32 rounding).
    The values are not integers: a sharded round is refused (``fractional_values``).  ``objective`` turns a round's value into the
    reference's -(min_res + sca)."""

    num_edges = 0
    value_scale = 0.5
    fractional_values = True      # MCPGRound: no integer MAXLOC key exists for these values, a sharded round is refused

    @property
    def Sigma(self) -> TEN:
        return self[0]

    @property
    def Diag(self) -> TEN:
        return self[1]

    def local_search(self, xs: PackedChains, num_ls: int, out=None, num_chains: Optional[int] = None):
        """Sweeps + value on bit-packed chains: (chains after the sweeps, expected f32 [C])."""
        return mops.mcpg_mimo_local_search(self[0], self[1], xs, num_ls, out=out, num_chains=num_chains)

    def round_local_search(self, samples: PackedChains, num_ls: int, seed: int, out: PackedChains, chain_ids):
        """What MCPGRound calls in place of the MaxCut kernel: (chains, 2 expected).  Nothing is drawn: seed and chain_ids are unused."""
        xs, expected = self.local_search(samples, num_ls, out=out)
        return xs, expected * 2

    def result(self, xs) -> TEN:
        """-expected f32 [C] of chains taken as +-1 (f32 [n, C] holding 0|1, or PackedChains), nothing swept -- the incumbents' values
        run_mcpg starts from."""
        packed = xs if isinstance(xs, PackedChains) else PackedChains.pack(xs.to(self.device, torch.float32).contiguous())
        _, expected = mops.mcpg_mimo_local_search(self[0], self[1], packed, 0, _score_only=True)
        return -expected

    def objective(self, value: float) -> float:
        """A round's value (-expected of a chain) -> the reference's -(min_res + sca) = -|Y - H x|^2."""
        return float(value) - float(self[3])


def supported_limit(num_chains: int = 0) -> int:
    """Largest n the kernel covers at this many chains (rls_mimo_local_search_supported: the bit tile + the partial tiles in LDS)."""
    lo, hi = 1, 1 << 17
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if mops.mimo_launch_form(mid, num_chains)[0]:
            lo = mid
        else:
            hi = mid - 1
    return lo


def make_data(Sigma, Diag, X, sca, noise, device) -> Data_MIMO:
    """The data object of an instance given as arrays (numpy or torch, any float type): Sigma [n, n], Diag [n], X [n], sca, noise.
    Raises ValueError naming the limit for data the kernel does not take."""
    S = np.asarray(Sigma.detach().cpu() if isinstance(Sigma, torch.Tensor) else Sigma, dtype=np.float64)
    D = np.asarray(Diag.detach().cpu() if isinstance(Diag, torch.Tensor) else Diag, dtype=np.float64)
    Xn = np.asarray(X.detach().cpu() if isinstance(X, torch.Tensor) else X, dtype=np.float64)
    if S.ndim != 2 or S.shape[0] != S.shape[1] or S.shape[0] < 1:
        raise ValueError(f"Sigma must be square [n, n] with n >= 1, got {S.shape}")
    n = S.shape[0]
    if D.shape != (n,):
        raise ValueError(f"Diag must be [{n}] (Sigma is [{n}, {n}]), got {D.shape}")
    if Xn.shape != (n,):
        raise ValueError(f"X must be [{n}] (Sigma is [{n}, {n}]), got {Xn.shape}")
    S32, D32 = S.astype(np.float32), D.astype(np.float32)
    sca_f, noise_f = float(sca), float(noise)
    if not (np.isfinite(S32).all() and np.isfinite(D32).all() and np.isfinite(sca_f) and np.isfinite(noise_f)):
        raise ValueError("Sigma, Diag, sca and noise must be finite in float32")
    if not mops.mimo_launch_form(n, 0)[0]:
        raise ValueError(f"the MIMO sampler covers 1 <= n <= {supported_limit()} variables (the bit tile in LDS); got n={n}")
    device = torch.device(device)
    data = Data_MIMO([torch.from_numpy(S32).to(device), torch.from_numpy(D32).to(device), torch.from_numpy(Xn).to(device),
                      torch.tensor(sca_f, dtype=torch.float64, device=device), noise_f])
    data.num_nodes, data.device = n, device
    return data


# ------------------------------------------------------------------------------ instances and the two file forms
def mimo_instance(K: int, N: int, SNR: float, seed: int, integer: bool = False) -> dict:
    """A seeded instance of K users and N antennas as the real-valued system the loaders read: dict(K, SNR, H [2N, 2K] standard
    normal, X [2K] uniform in {-1, +1}, v [2N] standard normal, not yet scaled).  ``integer``: H in {-3..3} and v in {-2..2} --
    with the loaders' ``noise_scale=1`` Sigma, Diag and sca are then integers, and the kernel is bit-exact with the reference."""
    g = np.random.default_rng(seed)
    if integer:
        H = g.integers(-3, 4, size=(2 * N, 2 * K)).astype(np.float64)
        v = g.integers(-2, 3, size=2 * N).astype(np.float64)
    else:
        H = g.standard_normal((2 * N, 2 * K))
        v = g.standard_normal(2 * N)
    X = g.integers(0, 2, size=2 * K) * 2.0 - 1.0
    return dict(K=int(K), SNR=float(SNR), H=H, X=X, v=v)


def instance_arrays(H, X, v, K, SNR, noise_scale: Optional[float] = None):
    """dataloader.py:343-353 / :377-387 in float64: (Sigma, Diag, X, sca, noise).  ``noise_scale`` replaces the factor
    sqrt(2 K 10^(-SNR / 10)) on v (1 for the integer instances)."""
    H, X, v = np.asarray(H, dtype=np.float64), np.asarray(X, dtype=np.float64), np.asarray(v, dtype=np.float64)
    if H.ndim != 2 or X.shape != (H.shape[1],) or v.shape != (H.shape[0],):
        raise ValueError(f"H must be [rows, cols] with X [cols] and v [rows]; got H {H.shape}, X {X.shape}, v {v.shape}")
    v = (np.sqrt(2 * K * 10 ** (-SNR / 10)) if noise_scale is None else noise_scale) * v
    Y = H.dot(X) + v
    noise = np.linalg.norm(v)
    Sigma = H.T.dot(H)
    Diag = -2 * Y.T.dot(H)
    sca = Y.T.dot(Y)
    for i in range(Sigma.shape[0]):
        sca += Sigma[i][i]
        Sigma[i][i] = 0
    return Sigma, Diag, X, sca, noise


def data_from_instance(inst: dict, device, noise_scale: Optional[float] = None) -> Data_MIMO:
    """The data object of a mimo_instance dict, as the loaders build it from a file."""
    return make_data(*instance_arrays(inst["H"], inst["X"], inst["v"], int(inst["K"]), float(inst["SNR"]), noise_scale), device)


def _fmt(row) -> str:
    return ", ".join(repr(float(a)) for a in row)


def write_mimo3(path: str, inst: dict) -> None:
    """The text form read_data_mimo3 reads: SNR, K, H (line j = COLUMN j of H), v, X."""
    H = np.asarray(inst["H"], dtype=np.float64)
    lines = ["SNR", repr(float(inst["SNR"])), "K", str(int(inst["K"])), "H"] + [_fmt(H[:, j]) for j in range(H.shape[1])]
    lines += ["v", _fmt(inst["v"]), "X", _fmt(inst["X"])]
    with open(path, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


def write_mimo5(path: str, inst: dict) -> None:
    """The npz form read_data_mimo5 reads (K, SNR, H, X, v)."""
    np.savez(path, K=np.int64(inst["K"]), SNR=np.float64(inst["SNR"]), H=np.asarray(inst["H"], dtype=np.float64),
             X=np.asarray(inst["X"], dtype=np.float64), v=np.asarray(inst["v"], dtype=np.float64))


def _numbers(line: str, what: str):
    try:
        return [float(m) for m in line.replace("\n", "").split(", ") if len(m) >= 1]
    except ValueError as e:
        raise ValueError(f"MIMO file: the {what} line holds something that is no number ({e})") from None


def parse_mimo3(text_lines) -> dict:
    """The sections of the text form -> dict(K, SNR, H, X, v); ValueError on a missing section or a ragged H."""
    it = iter(text_lines)
    SNR = K = H = v = X = None
    for line in it:
        line = line.replace("\n", "")
        if line == "SNR":
            SNR = _numbers(next(it, ""), "SNR")
            SNR = SNR[0] if len(SNR) == 1 else None
        elif line == "K":
            try:
                K = int(next(it, ""))
            except ValueError:
                raise ValueError("MIMO file: the line after 'K' must hold one integer") from None
        elif line == "H":
            if K is None or K < 1:
                raise ValueError("MIMO file: section K must come before section H and be >= 1")
            cols = [_numbers(next(it, ""), f"H column {j}") for j in range(2 * K)]
            if len(cols[0]) == 0 or any(len(c) != len(cols[0]) for c in cols):
                raise ValueError(f"MIMO file: the {2 * K} lines of section H must hold one column of H each, all of one length; got lengths "
                                 f"{sorted(set(len(c) for c in cols))}")
            H = np.array(cols, dtype=np.float64).T
        elif line == "v":
            v = np.array(_numbers(next(it, ""), "v"))
        elif line == "X":
            X = np.array(_numbers(next(it, ""), "X"))
            break
    missing = [name for name, val in (("SNR", SNR), ("K", K), ("H", H), ("v", v), ("X", X)) if val is None]
    if missing:
        raise ValueError(f"MIMO file: section(s) {', '.join(missing)} missing")
    return dict(K=K, SNR=SNR, H=H, X=X, v=v)


def read_data_mimo3(filename: str, X_num, r_seed, device=None, noise_scale: Optional[float] = None) -> Data_MIMO:
    """dataloader.py:297-362: the text form.  ``X_num`` / ``r_seed`` are accepted and unused, as there.  H is rounded to float32
    as there (the reference then forms Sigma = H^T H in float32; here every product is float64 and the cast comes last)."""
    with open(filename, "r", encoding="utf-8") as f:
        inst = parse_mimo3(f)
    inst["H"] = inst["H"].astype(np.float32).astype(np.float64)      # the reference parses H through float32 tensors (:324)
    return data_from_instance(inst, _device(device), noise_scale)


def read_data_mimo5(K: int, N: int, SNR: float, X_num: int, r_seed: int, device=None, data_dir: Optional[str] = None,
                    noise_scale: Optional[float] = None) -> Data_MIMO:
    """dataloader.py:365-396: <data_dir>/4QAM{N}_{K}/4QAM{K}_{r_seed // X_num + 1}.npz.  The noise scale uses the ARGUMENTS K and
    SNR, not the file's, as the reference does."""
    ident = int(r_seed // X_num + 1)
    filename = os.path.join("data/MIMO" if data_dir is None else data_dir, "4QAM{}_{}".format(N, K), "4QAM{}_{}.npz".format(K, ident))
    with np.load(filename) as z:
        missing = [k for k in ("K", "SNR", "H", "X", "v") if k not in z.files]
        if missing:
            raise ValueError(f"{filename}: array(s) {', '.join(missing)} missing")
        H, X, v = z["H"], z["X"], z["v"]
    return make_data(*instance_arrays(H, X, v, K, SNR, noise_scale), _device(device))


def _device(device):
    return torch.device("cuda" if device is None else device)


# ------------------------------------------------------------------------------ the samplers
def sampler_mimo_packed(data: Data_MIMO, xs: PackedChains, num_ls: int, total_mcmc_num: int, repeat_times: int,
                        num_chains: Optional[int] = None, in_place: bool = True):
    """Sweeps, value and best of repeats on bit-packed chains.  Returns (-(expected[best] + sca) f32 [M], best PackedChains of M
    chains, value f32 [C] = expected - mean(expected), chains after the sweeps)."""
    Cc = xs.num_chains if num_chains is None else num_chains
    out = xs if (in_place and xs.num_chains == Cc) else PackedChains.empty(xs.num_nodes, Cc, xs.device)
    xs_loc, expected = data.local_search(xs, num_ls, out=out, num_chains=Cc)
    _, best_val, best = mops.mcpg_pick_best(expected * 2, xs_loc, total_mcmc_num, repeat_times, 0)
    return best_val - data[3], best, value_of(expected), xs_loc


def mcpg_sampling_mimo(data: Data_MIMO, start_result: TEN, probs: TEN, num_ls: int, change_times: int, total_mcmc_num: int,
                       device=None, index: Optional[TEN] = None, u: Optional[TEN] = None):
    """sampling.py:288-320 -> (-(expected[best] + sca) f32 [M], chains of the best repeats f32 [n, M] holding 0|1, the metro output
    f32 [n, C], expected - mean f32 [C]).  ``index`` / ``u`` replace the walk's torch.randint / torch.rand draws (test hooks)."""
    device = data.device if device is None else torch.device(device)
    raw = metro_sampling(probs, start_result.to(device), change_times, device, index=index, u=u)
    Cc = raw.shape[1]
    packed = PackedChains.pack(raw)
    xs_loc, expected = data.local_search(packed, num_ls, out=packed)
    best_index, _, best = mops.mcpg_pick_best(expected * 2, xs_loc, total_mcmc_num, Cc // total_mcmc_num, 0)
    return -(expected[best_index] + data[3]), best.unpack(), raw, value_of(expected)


# ------------------------------------------------------------------------------ the driver's table and epilogue
_PARAMETERS = {   # (N = K, SNR) -> (num_ls, num_epochs, max_range), MCPG.py:112-169
    800: {2: (3, 1, 150), 4: (3, 2, 150), 6: (5, 5, 150), 8: (7, 3, 150), 10: (5, 2, 150), 12: (4, 2, 150)},
    1000: {2: (2, 2, 150), 4: (3, 2, 150), 6: (7, 4, 150), 8: (8, 4, 150), 10: (7, 2, 150), 12: (3, 3, 150)},
    1200: {2: (3, 1, 150), 4: (3, 2, 150), 6: (7, 3, 150), 8: (6, 4, 100), 10: (4, 4, 150), 12: (5, 2, 150)},
}


def mimo_parameters(SNR, N: int, K: int):
    """get_parameter of MCPG.py:108-171 -> (num_ls, num_epochs, max_range); (4, 3, 150) off the table."""
    if N == K and N in _PARAMETERS and SNR in _PARAMETERS[N]:
        return _PARAMETERS[N][SNR]
    return 4, 3, 150


def mimo_vote(now_max_res: TEN, now_max_info: TEN, max_range: int) -> TEN:
    """MCPG.py:184-192: the sign of (best chain + the ``max_range`` best chains), chains as +-1 -- the best chain counts twice, as
    there.  now_max_res [M], now_max_info [n, M] holding 0|1; ``max_range`` is capped at M (the reference would index past the
    end).  Returns f32 [n] in {-1, 0, +1}."""
    res = torch.as_tensor(now_max_res)
    info = torch.as_tensor(now_max_info).to(torch.float32) * 2 - 1
    order = torch.argsort(res, descending=True, stable=True)
    k = min(int(max_range), order.shape[0])
    total = info[:, order[0]] + info[:, order[:k]].sum(dim=1)
    return torch.sign(total)


def bit_error_rate(x, X) -> float:
    """MCPG.py:193: the share of positions where x differs from the sent symbols X."""
    x, X = torch.as_tensor(x).detach().cpu().to(torch.float64), torch.as_tensor(X).detach().cpu().to(torch.float64)
    return float((x != X).sum().item()) / X.numel()
