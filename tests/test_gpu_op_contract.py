"""The contract of csrc/torch_ops.cpp, op by op: "an op checks device / dtype / contiguity AND every shape against the graph handle and
the other arguments (a wrongly shaped tensor is a TORCH_CHECK here, never a device out-of-bounds access)".

1. Completeness: tests/op_contract.py has one valid call for every device entry point.
2. The refusal sweep: for every op, every Tensor argument of its valid call is replaced in turn by a tensor of a wrong dtype, a
   non-contiguous one, one that is one element / row / column short, and a host tensor (a device one for the host-side row_index).  Every such call
   must raise and must leave every byte the test owns as it was.  What the contract accepts on purpose is listed in EXEMPT with the
   line that says so; an accepted call must reproduce the valid call's outputs.  Range-checked int arguments (SCALARS) likewise.
3. The indices kernels read from DEVICE memory, at the edges of their ranges, against numpy restatements: exact.

Every device tensor of a call is a view into one allocation the test owns, with a band of guard bytes on both sides; a mutated
tensor keeps the bytes of the whole original behind its view, followed by a band as large.  So if a check is missing and the
kernel runs, it reads what the valid call read and writes memory the test owns: the cell fails on a changed output or guard, not
on a fault.  No wild pointer, no freed tensor, no far-off index."""
import numpy as np
import pytest
import torch

from tests import op_contract as oc

gpu = pytest.mark.gpu
PAD, CANARY, OTHER = 256, 0xA5, 0x3C
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def test_the_table_has_one_row_per_device_entry_point():
    from rlsolver_amd import torch_ops
    want, have = set(torch_ops.DEVICE_ENTRY_POINTS), set(oc.ROWS)
    assert not want - have, f"device entry points without a row in tests/op_contract.py: {sorted(want - have)}"
    assert not have - want, f"rows of tests/op_contract.py that are no device entry point: {sorted(have - want)}"
    for op, r in oc.ROWS.items():
        assert set(r.outs) <= set(oc.written(op)), op


# ---------------------------------------------------------------------------------------------------------------- guard bands
def _up(n):
    return (n + PAD - 1) // PAD * PAD


def _nbytes(t):
    return t.numel() * t.element_size()


def _raw(t):
    """the bytes of a tensor, contiguous, as uint8 [nbytes] (a copy)"""
    return t.contiguous().reshape(-1).view(torch.uint8).clone() if t.numel() else torch.empty(0, dtype=torch.uint8, device=t.device)


class Arena:
    """Every tensor of `tensors` as a view into ONE buffer: [band | tensor | band] each, the bands filled with CANARY and at least
    as long as the tensor they surround.  `fill`: names whose tensor starts as CANARY bytes too (results nobody reads)."""

    def __init__(self, tensors, fill=()):
        self.slots, off = {}, 0
        for name, t in tensors.items():
            band = _up(_nbytes(t)) + PAD
            self.slots[name] = (off + band, _nbytes(t))
            off += band + _up(_nbytes(t)) + band
        self.buf = torch.full((max(off, PAD),), CANARY, dtype=torch.uint8, device=oc.DEV)
        self.is_band = torch.ones(self.buf.numel(), dtype=torch.bool, device=oc.DEV)
        self.views = {}
        for name, t in tensors.items():
            start, nb = self.slots[name]
            self.is_band[start:start + nb] = False
            if name not in fill:
                self.buf[start:start + nb] = _raw(t)
            self.views[name] = self.buf[start:start + nb].view(t.dtype).reshape(t.shape)
            assert self.views[name].is_contiguous() and self.views[name].data_ptr() % 16 == 0

    def body(self, snapshot, name):
        start, nb = self.slots[name]
        return snapshot[start:start + nb]

    def bands_intact(self):
        return bool(self.buf[self.is_band].eq(CANARY).all())


class Mutant:
    """One replaced tensor: `view` over `body` bytes inside [band | body | band]; the body keeps the bytes of the whole original."""

    def __init__(self, body, make_view):
        n = body.numel()
        band = _up(n) + PAD
        self.buf = torch.full((band + _up(n) + band,), CANARY, dtype=torch.uint8, device=body.device)
        self.buf[band:band + n] = body
        self.view = make_view(self.buf[band:band + n])
        self.lo, self.hi = band, band + n
        self.snapshot = self.buf.clone()

    def intact(self):
        return torch.equal(self.buf, self.snapshot)

    def bands_intact(self):
        return bool(self.buf[:self.lo].eq(CANARY).all()) and bool(self.buf[self.hi:].eq(CANARY).all())


def _wrong_dtype(dt):
    return torch.float64 if dt == torch.float16 else torch.float16       # no argument of any op takes it in place of `dt`


def mutation_plan(t):
    """name -> a function that builds the Mutant (or, for the move to the other side, the bare tensor), for every mutation that applies to `t`"""
    plan, n, shape = {}, t.numel(), tuple(t.shape)

    def dtype():
        nd = _wrong_dtype(t.dtype)
        nes, raw = torch.empty((), dtype=nd).element_size(), _raw(t)
        body = torch.cat([raw, torch.zeros(max(0, n * nes - raw.numel()), dtype=torch.uint8, device=raw.device)])
        return Mutant(body, lambda b: b[:n * nes].view(nd).reshape(shape))

    def noncontiguous():
        raw, strides = _raw(t), [2 * s for s in t.contiguous().stride()]
        m = Mutant(torch.cat([raw, raw]), lambda b: torch.as_strided(b.view(t.dtype), shape, strides))
        assert not m.view.is_contiguous()
        return m

    def short(cut):
        def build():
            cshape, craw, body = tuple(cut.shape), _raw(cut), _raw(t)
            body[:craw.numel()] = craw
            return Mutant(body, lambda b: b[:craw.numel()].view(t.dtype).reshape(cshape))
        return build

    if n:
        plan["dtype"] = dtype
    if n >= 2:
        plan["noncontiguous"] = noncontiguous
    if t.dim() == 1 and shape[0] >= 1:
        plan["short"] = short(t[:-1])
    elif t.dim() >= 2:
        if shape[0] >= 1:
            plan["short_row"] = short(t[:-1])
        if shape[-1] >= 1:
            plan["short_col"] = short(t[..., :-1])
    plan["other_side"] = lambda: t.cpu() if t.is_cuda else t.to(oc.DEV)
    return plan


def mutants(t):
    return {kind: build() for kind, build in mutation_plan(t).items()}


# ---------------------------------------------------------------------------------------------------------------- what the contract accepts
# (op, argument, mutation) -> (file, a snippet of the line that allows it, quoted verbatim; whether the call is ANOTHER problem).
# An exempt cell must NOT raise and must reproduce the valid call's outputs -- unless the tensor itself defines the problem's size
# (sizes()): then the call is a smaller problem, and "does not raise, every guard band intact" is what can be asked of it.
OPS_CPP, HEADER = "rlsolver_amd/csrc/torch_ops.cpp", "include/rlsolver_hip.h"


def sizes(snippet):
    return (OPS_CPP, snippet, True)


SCRATCH_ANY_SIZE = (HEADER, "With scratch = NULL (or too small) both run one workgroup per tile; the results are the same either way", False)
ISCO_SCRATCH = (HEADER, "0 (scratch may be NULL) while a sample's rows fit LDS", False)
ANY_DTYPE = (OPS_CPP, 'dev(*scratch, "scratch");', False)
EXEMPT = {
    ("maxcut_ls_normals", "out", "short_row"): sizes("rls_maxcut_ls_normals((float*)p(out), out.size(0), out.size(1)"),
    ("maxcut_ls_normals", "out", "short_col"): sizes("rls_maxcut_ls_normals((float*)p(out), out.size(0), out.size(1)"),
    ("rand_spins", "x", "short_row"): sizes("rls_rand_spins((uint8_t*)p(x), x.size(0), x.size(1)"),
    ("rand_spins", "x", "short_col"): sizes("rls_rand_spins((uint8_t*)p(x), x.size(0), x.size(1)"),
    ("rand_actions", "action", "short"): sizes("rls_rand_actions((int64_t*)p(action), action.numel()"),
    ("rand_perms", "perm", "short_row"): sizes("rls_rand_perms((int64_t*)p(perm), perm.size(0), perm.size(1)"),
    ("rand_perms", "perm", "short_col"): sizes("rls_rand_perms((int64_t*)p(perm), perm.size(0), perm.size(1)"),
    ("rand_couplings", "matrix", "short_row"): sizes("matrix.size(0), matrix.size(1), (int32_t)kind"),
    ("rand_spins_repeats", "x", "short_col"): sizes("rls_rand_spins_repeats((uint8_t*)p(x), x.size(0), x.size(1), x.size(2)"),
    ("best_key", "vs", "short"): sizes("rls_best_key(p(vs), kind, vs.numel()"),
    ("copy_rows", "xs", "short_col"): sizes("xs.size(0), xs.size(1), (const int64_t*)p(dst)"),
    ("copy_rows_bounded", "xs", "short_col"): sizes("xs.size(0), xs.size(1), (const int64_t*)p(dst)"),
    ("winner_message", "xs", "short_row"): sizes("B = xs->dim() == 2 ? xs->size(0) : 1;"),
    ("s2vppo_reset", "ids", "short"): sizes("ids.has_value() ? ids->numel() : e.num_envs"),
    ("mcpg_metro_stop", "accepts", "short_row"): sizes("accepts.size(0), accepts.size(1), target"),
    ("mcpg_metro_stop", "accepts", "short_col"): sizes("accepts.size(0), accepts.size(1), target"),
    ("mcpg_local_search", "visit_stream", "short"): sizes("visit_stream.has_value() ? visit_stream->numel() : 0"),
    ("mcpg_local_search_levels", "lv_ptr", "short"): sizes("lv_ptr.numel() - 1, num_ls"),
    ("maxsat_local_search", "lv_ptr", "short"): sizes("(const int32_t*)p(lv_data), lv_ptr.numel() - 1,"),
    ("maxsat_local_search", "clause_ptr", "short"): sizes("const int64_t M = clause_ptr.numel() - 1;"),
    ("qubo_sparse_local_search_value", "lv_ptr", "short"): sizes("lv_ptr->numel() - 1"),
    # the caller's contract, stated in the header beside the tours of the TSP ops: lengths only device memory holds
    ("mcpg_local_search_levels", "lv_data", "short"): (HEADER, "lv_data holds the `total` entries that lv_ptr's offsets name", False),
    ("maxsat_local_search", "lv_data", "short"): (HEADER, "lv_data holds the `total` entries of rls_maxsat_visit_levels and lit the clause_ptr[M]", False),
    ("maxsat_local_search", "lit", "short"): (HEADER, "lv_data holds the `total` entries of rls_maxsat_visit_levels and lit the clause_ptr[M]", False),
    # accepted on purpose
    ("maxcut_edge_local_search", "visit_stream", "short"): (OPS_CPP, "visit_stream must be 1-D and hold at least 7 E = ", False),
    ("maxcut_ls_weights", "ws", "short_col"): (OPS_CPP, "ws [B, pitch >= N] contiguous: entries N .. pitch of a row are padding", False),
    ("maxcut_ls_threshold", "scratch", "short"): SCRATCH_ANY_SIZE,
    ("maxcut_ls_propose", "scratch", "short"): SCRATCH_ANY_SIZE,
    ("maxcut_ls_rounds", "scratch", "short"): SCRATCH_ANY_SIZE,
    ("mcpg_metro_rounds", "scratch", "short"): (HEADER, "`scratch` (device, may be NULL) of at least rls_mcpg_metro_scratch_bytes(N, C) bytes lets", False),
    ("mcpg_metro_rounds", "scratch", "dtype"): ANY_DTYPE,
    ("isco_maxcut_step", "scratch", "short"): ISCO_SCRATCH,
    ("isco_maxcut_step", "scratch", "dtype"): ANY_DTYPE,
    ("isco_mis_step", "scratch", "short"): ISCO_SCRATCH,
    ("isco_mis_step", "scratch", "dtype"): ANY_DTYPE,
    ("pisco_step", "scratch", "dtype"): (OPS_CPP, 'dev(scratch, "scratch");', False),
}
_OTHER_PROBLEM = {k for k, v in EXEMPT.items() if v[2]}
# (row, argument, mutation) an exemption of the op does not reach in that row, and the check that refuses it there
REFUSED_IN_ROW = {("maxsat_local_search#weighted", "clause_ptr", "short"): "count(*weight, \"weight\", M): with weights, M is held against them"}
# Tensor arguments no row passes, with the reason (the sweep cannot mutate what is not there)
NOT_MUTATED = {}


def test_every_exemption_quotes_a_line_that_is_still_there():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = {f: " ".join(open(os.path.join(root, f)).read().split()) for f in (OPS_CPP, HEADER)}
    for (op, arg, kind), (where, snippet, _) in EXEMPT.items():
        assert op in oc.ROWS and arg in oc.tensor_names(op), (op, arg)
        assert " ".join(snippet.split()) in text[where], f"{op}.{arg}/{kind}: {where} no longer says: {snippet}"
    for op in oc.ROWS:                                          # no op is exempt as a whole
        cells = {(a, k) for (o, a, k) in EXEMPT if o == op}
        assert len(cells) < 3 * max(1, len(oc.tensor_names(op))), op


@gpu
def test_every_tensor_argument_is_mutated_in_some_row_and_every_exemption_is_reached():
    """A `Tensor?` a row passes as None is not mutated by that row: another row of the op must pass it."""
    seen = {}
    for key, r in oc.ALL.items():
        args, _, _ = r.valid_call()
        for n, a in zip(oc.names(r.op), args):
            if isinstance(a, torch.Tensor):
                seen.setdefault((r.op, n), set()).update(mutation_plan(a))
    missing = [(op, n) for op in oc.ROWS for n in oc.tensor_names(op) if (op, n) not in seen and (op, n) not in NOT_MUTATED]
    assert not missing, f"tensor arguments no row of tests/op_contract.py passes: {missing}"
    assert not [k for k in NOT_MUTATED if k in seen], "NOT_MUTATED lists an argument a row does pass"
    unreached = [k for k in EXEMPT if k[2] not in seen.get(k[:2], ())]
    assert not unreached, f"exemptions no row reaches: {unreached}"


# ---------------------------------------------------------------------------------------------------------------- the sweep
class Valid:
    """The valid call of an op inside an Arena: `base` its arguments, `initial` / `after` the arena before / after it."""

    def __init__(self, key):
        self.row = oc.ALL[key]
        self.op = op = self.row.op
        args, self.written, fix = self.row.valid_call()
        self.names = oc.names(op)
        dev_t = {n: a for n, a in zip(self.names, args) if isinstance(a, torch.Tensor) and a.is_cuda}
        spans = sorted((a.data_ptr(), a.data_ptr() + _nbytes(a), n) for n, a in dev_t.items() if a.numel())
        for (_, hi, n0), (lo, _, n1) in zip(spans, spans[1:]):
            assert hi <= lo, f"{op}: {n0} and {n1} of the valid call share bytes"
        self.arena = Arena(dev_t, fill=self.row.outs)
        self.base = [self.arena.views.get(n, a) if isinstance(a, torch.Tensor) else a for n, a in zip(self.names, args)]
        if fix is not None:
            self.base, self.keep = fix(op, self.base), fix
        self.initial = self.arena.buf.clone()
        oc.call(op, self.base)
        torch.cuda.synchronize()
        self.after = self.arena.buf.clone()
        assert self.arena.bands_intact(), f"{op}: the VALID call wrote outside its arguments"
        assert not torch.equal(self.after, self.initial), f"{op}: the valid call changed nothing: the sweep would be blind"
        for n in self.row.outs:
            if n in self.arena.slots and self.arena.slots[n][1]:
                assert not torch.equal(self.arena.body(self.after, n), self.arena.body(self.initial, n)), f"{op}: output {n} was not written"

    def restore(self):
        self.arena.buf.copy_(self.initial)

    def same_results(self, skip=()):
        """names of written arguments whose bytes differ from the valid call's"""
        now = self.arena.buf
        return [n for n in self.written if n in self.arena.slots and n not in skip
                and not torch.equal(self.arena.body(now, n), self.arena.body(self.after, n))]


@gpu
@pytest.mark.parametrize("op", sorted(oc.ALL))
def test_outputs_are_results_only_and_the_valid_call_repeats(op):
    """What a row lists as `outs` is filled with a pattern before every call of the sweep: the op must not read it.  The valid call
    from another pattern gives the same bytes everywhere."""
    v = Valid(op)
    if not v.row.repeatable:
        return
    v.restore()
    for n in v.row.outs:
        if n in v.arena.slots:
            start, nb = v.arena.slots[n]
            v.arena.buf[start:start + nb] = OTHER
    oc.call(v.op, v.base)
    torch.cuda.synchronize()
    assert v.same_results() == [] and v.arena.bands_intact()


@gpu
@pytest.mark.parametrize("op", sorted(oc.ALL))
def test_every_mutated_tensor_argument_is_refused(op):
    key, v = op, Valid(op)
    op = v.op
    failures, cells = [], 0
    for i, name in enumerate(v.names):
        arg = v.base[i]
        if not isinstance(arg, torch.Tensor):
            continue
        v.restore()
        for kind, m in mutants(arg).items():
            cells += 1
            cell, exempt = f"{key}.{name}/{kind}", (op, name, kind) in EXEMPT and (key, name, kind) not in REFUSED_IN_ROW
            v.restore()
            args = list(v.base)
            args[i] = m.view if isinstance(m, Mutant) else m
            try:
                oc.call(op, args)
                raised = None
            except RuntimeError as e:                       # (NotImplementedError, the dispatcher's, is one)
                raised = e
            torch.cuda.synchronize()
            m_ok = m.intact() if isinstance(m, Mutant) else True
            if exempt:
                if raised is not None:
                    failures.append(f"{cell}: exempt, but refused ({str(raised).splitlines()[0][:120]}): drop the exemption")
                elif not (v.arena.bands_intact() and (not isinstance(m, Mutant) or m.bands_intact())):
                    failures.append(f"{cell}: exempt, and a guard band changed")
                elif (op, name, kind) not in _OTHER_PROBLEM and v.same_results(skip=(name,)):
                    failures.append(f"{cell}: exempt, but {v.same_results(skip=(name,))} differ from the valid call's")
                continue
            if raised is None:
                changed = "outputs or guards changed" if not (torch.equal(v.arena.buf, v.initial) and m_ok) else "nothing the test owns changed"
                failures.append(f"{cell}: accepted ({changed})")
            elif not torch.equal(v.arena.buf, v.initial):
                failures.append(f"{cell}: refused, but an argument or a guard band changed first")
            elif not m_ok:
                failures.append(f"{cell}: refused, but the mutated tensor or its guard band changed first")
    assert cells >= 4, op
    assert not failures, f"{len(failures)} of {cells} cells:\n" + "\n".join(failures)


# ---- the dtype alternatives the contract names: the same results, byte for byte
@gpu
@pytest.mark.parametrize("op", sorted(oc.ALL))
def test_bool_arguments_given_as_uint8_give_the_same_bytes(op):
    """torch_ops.cpp spin_bytes: "spins: bool / uint8 (1 byte)" -- every bool tensor of the valid call as its uint8 view"""
    v = Valid(op)
    at = [i for i, a in enumerate(v.base) if isinstance(a, torch.Tensor) and a.dtype == torch.bool]
    if not at or not v.row.repeatable:
        return
    v.restore()
    args = list(v.base)
    for i in at:
        args[i] = args[i].view(torch.uint8)
    oc.call(v.op, args)
    torch.cuda.synchronize()
    assert torch.equal(v.arena.buf, v.after)


# (op, the spin arguments that may be float32 together, the line that says so)
F32_SPINS = [("maxcut_obj", ("xs",), "torch_ops.cpp maxcut_obj: spin_bytes(xs, \"xs\", true) -- bool / uint8 / float32"),
             ("maxcut_step", ("x_in", "x_out"), "torch_ops.cpp maxcut_step: spin_bytes(x_in, \"x_in\", true), x_out of the same dtype")]


@gpu
@pytest.mark.parametrize("op,spin_args,where", F32_SPINS)
def test_spins_given_as_float32_give_the_same_results(op, spin_args, where):
    v = Valid(op)
    v.restore()
    f32 = Arena({n: v.base[v.names.index(n)].to(torch.float32) for n in spin_args})
    args = list(v.base)
    for n in spin_args:
        args[v.names.index(n)] = f32.views[n]
    oc.call(op, args)
    torch.cuda.synchronize()
    assert v.arena.bands_intact() and f32.bands_intact(), where
    assert v.same_results(skip=spin_args) == [], where
    for n in spin_args:
        if n in v.written:
            want = v.arena.body(v.after, n).view(torch.bool).to(torch.float32)
            assert torch.equal(f32.views[n].reshape(-1), want), (n, where)


# ---------------------------------------------------------------------------------------------------------------- scalars
# (op, {argument: first value outside its range}, where the range is written)
_KEYS = "csrc/rls_track.hip RLS_REQUIRE(rank_bits >= 0 && rank_bits < 32 && .. low_code >= 0 && low_code < (1ll << rank_bits) ..)"
_CHAIN = "torch_ops.cpp ChainIdsArg: chain_offset / chain_period / chain_skip must be >= 0"
SCALARS = [
    ("maxcut_local_search", {"num_spin": oc.LS_N}, "rls_localsearch.hip: num_spin >= 0 && num_spin + 1 <= kTopCap && num_spin < N"),
    ("maxcut_local_search", {"num_spin": -1}, "rls_localsearch.hip: num_spin >= 0"),
    ("maxcut_local_search", {"num_iters": -1}, "rls_localsearch.hip: B >= 0 && num_iters >= 0"),
    ("maxcut_ls_normals", {"draw": -1}, "rls_localsearch.hip: draw >= 0 && env_offset >= 0"),
    ("maxcut_ls_normals", {"env_offset": -1}, "rls_localsearch.hip: draw >= 0 && env_offset >= 0"),
    ("maxcut_ls_threshold", {"draw": -1}, "rls_localsearch.hip: B >= 0 && draw >= 0"),
    ("maxcut_ls_threshold", {"num_spin": oc.N}, "rls_localsearch.hip: num_spin < N"),
    ("maxcut_ls_propose", {"draw": -1}, "rls_localsearch.hip: B >= 0 && draw >= 0"),
    ("maxcut_ls_rounds", {"first_draw": -1}, "rls_localsearch.hip: first_draw >= 0 && num_draws >= 0"),
    ("maxcut_ls_rounds", {"num_draws": -1}, "rls_localsearch.hip: first_draw >= 0 && num_draws >= 0"),
    ("pick_best_of_repeats", {"R": 0}, "torch_ops.cpp: R > 0 && xs.size(0) % R == 0"),
    ("pick_best_of_repeats", {"R": 4}, "torch_ops.cpp: R > 0 && xs.size(0) % R == 0"),
    ("best_update", {"log_index": -1}, "torch_ops.cpp: log_index >= 0 && log_index < log_v->numel()"),
    ("best_update", {"log_index": 4}, "torch_ops.cpp: log_index >= 0 && log_index < log_v->numel()"),
    ("best_key", {"rank_bits": -1}, _KEYS), ("best_key", {"rank_bits": 32}, _KEYS),
    ("best_key", {"low_code": -1}, _KEYS), ("best_key", {"low_code": 1 << 20}, _KEYS),
    ("best_key", {"limit": 0}, "rls_track.hip: limit > 0 && limit <= (1ll << (62 - rank_bits))"),
    ("best_key", {"limit": (1 << 42) + 1}, "rls_track.hip: limit > 0 && limit <= (1ll << (62 - rank_bits))"),
    ("key_unpack", {"rank_bits": -1}, _KEYS), ("key_unpack", {"rank_bits": 32}, _KEYS),
    ("key_unpack", {"world": 0}, "rls_track.hip: world >= 1 && world <= (1ll << rank_bits)"),
    ("key_unpack", {"world": (1 << 20) + 1}, "rls_track.hip: world >= 1 && world <= (1ll << rank_bits)"),
    ("winner_message", {"rank_bits": -1}, _KEYS), ("winner_message", {"rank_bits": 32}, _KEYS),
    ("winner_message", {"my_low_code": -1}, _KEYS), ("winner_message", {"my_low_code": 1 << 20}, _KEYS),
    ("winner_message", {"N": oc.N + 8}, "torch_ops.cpp: msg must hold 8 + ceil(N / 8) bytes"),
    ("winner_message", {"N": oc.N - 8}, "torch_ops.cpp: msg must hold 8 + ceil(N / 8) bytes"),
    ("winner_unpack", {"N": oc.N + 8}, "torch_ops.cpp: msg must hold 8 + ceil(N / 8) bytes"),
    ("winner_unpack", {"N": 0}, "torch_ops.cpp: msg must hold 8 + ceil(N / 8) bytes"),
    ("sub_set_sampling", {"R": 0}, "torch_ops.cpp: num_repeats must be >= 1"),
    ("sub_set_sampling", {"top_k": -1}, "torch_ops.cpp: top_k must be >= 0"),
    ("sub_set_sampling", {"env_offset": -1}, "torch_ops.cpp: env_offset must be >= 0"),
    ("s2vppo_step", {"tenure": -1}, "torch_ops.cpp: tabu_tenure must be in [0, 2^31)"),
    ("s2vppo_step", {"multiplier": 0}, "torch_ops.cpp: episode_length_multiplier must be >= 1"),
    ("s2vppo_step", {"max_nodes": -1}, "torch_ops.cpp: max_nodes must be in [0, total_nodes]"),
    ("s2vppo_step", {"max_nodes": sum(oc.S2V_SIZES) + 1}, "torch_ops.cpp: max_nodes must be in [0, total_nodes]"),
    ("s2vppo_reset", {"tenure": -1}, "torch_ops.cpp: tabu_tenure must be in [0, 2^31)"),
    ("s2vppo_reset", {"multiplier": 0}, "torch_ops.cpp: episode_length_multiplier must be >= 1"),
    ("s2vppo_reset", {"max_nodes": sum(oc.S2V_SIZES) + 1}, "torch_ops.cpp: max_nodes must be in [0, total_nodes]"),
    ("s2vppo_reset", {"env_offset": -1}, "torch_ops.cpp: env_offset must be >= 0"),
    ("spin_observation", {"step_index": -1}, "torch_ops.cpp: step_index >= 0 && step_index < table_len"),
    ("spin_observation", {"step_index": 12}, "torch_ops.cpp: step_index >= 0 && step_index < table_len (max_steps + 2 = 12)"),
    ("spin_materialize", {"step_index": -1}, "torch_ops.cpp: step_index >= 0 && step_index < table_len"),
    ("spin_materialize", {"step_index": 12}, "torch_ops.cpp: step_index >= 0 && step_index < table_len (max_steps + 2 = 12)"),
    ("spin_step", {"hist_len": -1}, "torch_ops.cpp: hist_len >= 0"),
    ("spin_step", {"hist_len": 11}, "rls_spin.hip: hist_len >= 0 && hist_len + 1 < env->table_len (12)"),
    ("spin_step", {"reward_mode": 4}, "rls_spin.hip: reward_mode >= 0 && reward_mode <= 3"),
    ("spin_step", {"reward_mode": -1}, "rls_spin.hip: reward_mode >= 0 && reward_mode <= 3"),
    ("spin_step_dense", {"hist_len": -1}, "torch_ops.cpp: hist_len >= 0"),
    ("spin_step_dense", {"reward_mode": 4}, "rls_spin.hip: reward_mode >= 0 && reward_mode <= 3"),
    ("rand_couplings", {"kind": 2}, "rls_spin.hip: kind must be 0 or 1"),
    ("rand_couplings", {"kind": -1}, "rls_spin.hip: kind must be 0 or 1"),
    ("rand_couplings", {"edge_type": 0}, "rls_spin.hip: edge_type >= 1 && edge_type <= 3"),
    ("rand_couplings", {"edge_type": 4}, "rls_spin.hip: edge_type >= 1 && edge_type <= 3"),
    ("mcpg_metro_rounds", {"chain_offset": -1}, _CHAIN), ("mcpg_metro_rounds", {"chain_period": -1}, _CHAIN),
    ("mcpg_metro_rounds", {"chain_skip": -1}, _CHAIN),
    ("mcpg_metro_rounds", {"t_offset": 1}, "torch_ops.cpp: index must be [>= t_offset + T, C]"),
    ("mcpg_metro_rounds", {"C": oc.C + 1}, "torch_ops.cpp: chain_shape(samples, sb, N, C)"),
    ("mcpg_metro_rounds", {"T": -1}, "rls_mcpg.hip: N > 0 && C >= 0 && T >= 0 && t_offset >= 0"),
    ("mcpg_metro_rounds", {"t_offset": -1}, "rls_mcpg.hip: N > 0 && C >= 0 && T >= 0 && t_offset >= 0"),
    ("mcpg_metro_stop", {"target": -1}, "rls_mcpg.hip: accept_rows >= 1 && T >= 1 && next_T >= 0 && target >= 0"),
    ("mcpg_metro_stop", {"next_T": -1}, "rls_mcpg.hip: accept_rows >= 1 && T >= 1 && next_T >= 0 && target >= 0"),
    ("isco_tsp_step", {"path_length": -1}, "rls_isco.hip: N > 2 && N < (1 << 24) && B >= 0 && path_length >= 0"),
    ("qubo_local_search_value", {"num_ls": -1}, "rls_qubo.hip: n > 0 && C >= 0 && num_ls >= 0"),
    ("qubo_sparse_local_search_value", {"num_ls": -1}, "rls_qubo.hip: n > 0 && C >= 0 && num_ls >= 0"),
    ("mcpg_local_search", {"num_ls": -1}, "rls_mcpg.hip: C >= 0 && num_ls >= 0"),
    ("mcpg_local_search_levels", {"num_ls": -1}, "rls_mcpg.hip: C >= 0 && num_ls >= 0 && num_groups > 0"),
    ("mcpg_metro_stop", {"first": -1}, "torch_ops.cpp: first must be 0, 1 or 2"),
    ("mcpg_metro_stop", {"first": 3}, "torch_ops.cpp: first must be 0, 1 or 2"),
    ("mcpg_local_search", {"gauge_node": -2}, "torch_ops.cpp: gauge_node outside [-1, N)"),
    ("mcpg_local_search", {"gauge_node": oc.N}, "torch_ops.cpp: gauge_node outside [-1, N)"),
    ("mcpg_local_search", {"chain_offset": -1}, _CHAIN),
    ("mcpg_local_search_levels", {"chain_period": -1}, _CHAIN),
    ("mcpg_local_search_levels", {"C": oc.C + 1}, "torch_ops.cpp: chain_shape(xs_out, osb, N, C)"),
    ("maxsat_local_search", {"num_ls": -1}, "torch_ops.cpp: num_ls must be >= 0"),
    ("maxsat_local_search", {"chain_skip": -1}, _CHAIN),
    ("cheeger_local_search", {"normalized": 2}, "torch_ops.cpp: normalized must be 0 or 1"),
    ("cheeger_local_search", {"normalized": -1}, "torch_ops.cpp: normalized must be 0 or 1"),
    ("cheeger_local_search", {"num_ls": -1}, "torch_ops.cpp: num_ls must be >= 0"),
    ("cheeger_local_search", {"C": -1}, "torch_ops.cpp: C and C_in must be >= 0"),
    ("maxcut_edge_local_search", {"max_abs_degree": -1}, "torch_ops.cpp: max_abs_degree and weight_abs_sum must be >= 0"),
    ("maxcut_edge_local_search", {"weight_abs_sum": -1}, "torch_ops.cpp: max_abs_degree and weight_abs_sum must be >= 0"),
    ("maxcut_edge_local_search", {"gauge_node": -2}, "torch_ops.cpp: gauge_node must be a node or -1"),
    ("maxcut_edge_local_search", {"gauge_node": oc.N}, "torch_ops.cpp: gauge_node must be a node or -1"),
    ("maxcut_edge_local_search", {"num_ls": -1}, "torch_ops.cpp: num_ls must be >= 0"),
    ("mimo_local_search", {"num_ls": 0}, "torch_ops.cpp: num_ls must be >= 1 with xs_out"),
    ("mimo_local_search", {"C_in": -1}, "torch_ops.cpp: C and C_in must be >= 0"),
    ("mcpg_pick_best", {"total_mcmc_num": 0}, "torch_ops.cpp: total_mcmc_num and repeat_times must be positive"),
    ("mcpg_pick_best", {"repeat_times": 0}, "torch_ops.cpp: total_mcmc_num and repeat_times must be positive"),
    ("mcpg_merge_best", {"total_mcmc_num": 0}, "torch_ops.cpp: M > 0"),
]
SCALARS += [(op, {a: 0}, "torch_ops.cpp G() / SE(): null handle") for op in sorted(oc.ROWS) for a in ("graph", "env") if a in oc.kinds(op)]


@gpu
@pytest.mark.parametrize("op", sorted({s[0] for s in SCALARS}))
def test_int_arguments_outside_their_range_are_refused(op):
    v = Valid(op)
    failures = []
    for _, bad, where in (s for s in SCALARS if s[0] == op):
        v.restore()
        args = list(v.base)
        for a, val in bad.items():
            assert oc.kinds(op)[a] == "int", (op, a)
            args[v.names.index(a)] = val
        try:
            oc.call(op, args)
            failures.append(f"{op}({bad}): accepted; {where}")
        except RuntimeError:
            pass
        torch.cuda.synchronize()
        if not torch.equal(v.arena.buf, v.initial):
            failures.append(f"{op}({bad}): an argument or a guard band changed")
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------------------------- overlap
# (op, output, input, the line that forbids sharing bytes)
NO_OVERLAP = [
    ("sub_set_sampling", "probs_out", "probs", "rlsolver_hip.h: no input is modified and no output may alias an input"),
    ("isco_maxcut_step", "y_out", "x", "rls_isco.hip isco_step_launch: y_out must not alias x"),
    ("isco_mis_step", "y_out", "x", "rlsolver_hip.h rls_isco_mis_step: y_out must not alias x"),
    ("pisco_step", "y_out", "x", "rlsolver_hip.h rls_pisco_step: y_out must not alias x"),
    ("isco_tsp_step", "perm_out", "perm_in", "rlsolver_hip.h rls_isco_tsp_step: perm_out (must not alias perm_in)"),
]


@gpu
@pytest.mark.parametrize("op,out,inp,where", NO_OVERLAP)
def test_an_output_that_shares_bytes_with_an_input_is_refused(op, out, inp, where):
    v = Valid(op)
    v.restore()
    args = list(v.base)
    args[v.names.index(out)] = args[v.names.index(inp)]
    with pytest.raises(RuntimeError):
        oc.call(op, args)
    torch.cuda.synchronize()
    assert torch.equal(v.arena.buf, v.initial), where


@gpu
def test_k4_in_place_equals_out_of_place():
    """rlsolver_hip.h: "x_out may equal x_in (in-place: only the flipped byte is written"."""
    v = Valid("maxcut_step")
    want = {n: v.arena.body(v.after, n).clone() for n in v.written if n in v.arena.slots}
    v.restore()
    args = list(v.base)
    args[v.names.index("x_out")] = args[v.names.index("x_in")]
    oc.call("maxcut_step", args)
    torch.cuda.synchronize()
    assert v.arena.bands_intact()
    for n in want:
        got = v.arena.body(v.arena.buf, "x_in" if n == "x_out" else n)
        assert torch.equal(got, want[n]), n


@gpu
def test_packed_k7_in_place_equals_out_of_place():
    """rlsolver_hip.h: "bit-packed (0; then xs_out may alias a bit-packed xs_in)"."""
    mops, d = oc._mops(), oc.mcpg_data()
    coins = oc.t(oc.rng(9).randint(0, 1 << 62, size=(2 * oc.N, (oc.C + 63) // 64)).astype(np.int64))
    src = oc.packed()
    a, ea = mops.mcpg_local_search_levels(d.graph, src, d._lv_ptr, d._lv_data, 2, 0, coins=coins, out=mops.PackedChains.empty(oc.N, oc.C, oc.DEV))
    same = src.clone()
    b, eb = mops.mcpg_local_search_levels(d.graph, same, d._lv_ptr, d._lv_data, 2, 0, coins=coins, out=same)
    valid = (1 << (oc.C % 64)) - 1                     # bits past C in the last tile are nobody's
    wa, wb = a.words.clone(), b.words.clone()
    wa[-1] &= valid
    wb[-1] &= valid
    assert torch.equal(wa, wb) and torch.equal(ea, eb)


# ---------------------------------------------------------------------------------------------------------------- 3. device-held indices
def _i64(v):
    return torch.tensor(list(v), dtype=torch.int64, device=oc.DEV)


def _copy_rows_want(xs, vs, dst, src):
    rows = xs.shape[0]
    out_x, out_v = xs.copy(), None if vs is None else vs.copy()
    for d, s in zip(dst, src):
        if 0 <= d < rows and 0 <= s < rows:
            out_x[d] = xs[s]
            if vs is not None:
                out_v[d] = vs[s]
    return out_x, out_v


_ROWS = 7
_BAD = [(-1, 6), (6, -1), (_ROWS, 6), (0, _ROWS), (I64_MIN, 6), (0, I64_MIN)]
_MOVES = [[(0, 6)], [(6, 0)]] + [[m] for m in _BAD] + [[(0, 6), (1, 5), bad, (2, 4), (3, 5)] for bad in _BAD]


@gpu
@pytest.mark.parametrize("op", ["copy_rows", "copy_rows_bounded"])
@pytest.mark.parametrize("with_vs", [True, False])
@pytest.mark.parametrize("n,lead", [(64, 0), (70, 0), (64, 4)])
def test_copy_rows_skips_a_move_whose_index_is_outside_the_rows(op, with_vs, n, lead):
    """xs[dst[k]] = xs[src[k]] for the moves inside [0, B); a move with either index outside is skipped and the rows around xs stay
    as they were.  (64, 0): the 16-byte path; (70, 0) and a 64-byte row that starts 4 bytes into a line: the byte path.  Before the
    kernel was given B, dst = -1 wrote the row in front of xs and dst = B the row behind it: the guard bands here."""
    r = oc.rng(n + lead)
    xs0 = r.randint(0, 2, size=(_ROWS, n)).astype(np.uint8)
    vs0 = r.randint(-99, 99, size=_ROWS).astype(np.int64)
    for moves in _MOVES:
        flat = torch.full((lead + _ROWS * n,), CANARY, dtype=torch.uint8, device=oc.DEV)
        tensors = {"flat": flat, "vs": oc.t(vs0), "dst": _i64(m[0] for m in moves), "src": _i64(m[1] for m in moves)}
        a = Arena(tensors)
        xs = a.views["flat"][lead:].view(_ROWS, n)
        xs.copy_(oc.t(xs0))
        assert xs.data_ptr() % 16 == lead
        oc.call(op, [xs.view(torch.bool), a.views["vs"] if with_vs else None, a.views["dst"], a.views["src"]])
        torch.cuda.synchronize()
        want_x, want_v = _copy_rows_want(xs0, vs0, [m[0] for m in moves], [m[1] for m in moves])
        assert a.bands_intact() and bool(a.views["flat"][:lead].eq(CANARY).all()), moves
        assert np.array_equal(xs.cpu().numpy(), want_x), moves
        assert np.array_equal(a.views["vs"].cpu().numpy(), want_v if with_vs else vs0), moves


@gpu
def test_the_first_copy_rows_entry_point_copies_and_skips_a_negative_index():
    """rls_copy_rows is not told B (rlsolver_hip.h): through the C ABI, a good move copies and a move with a negative index is
    skipped; no op calls it any more."""
    from rlsolver_amd import _abi, ops
    n = 70
    r = oc.rng(n)
    xs0, vs0 = r.randint(0, 2, size=(_ROWS, n)).astype(np.uint8), r.randint(-99, 99, size=_ROWS).astype(np.int64)
    moves = [(0, 6), (-1, 5), (1, 5), (2, -1), (I64_MIN, 4), (3, I64_MIN)]
    a = Arena({"xs": oc.t(xs0), "vs": oc.t(vs0), "dst": _i64(m[0] for m in moves), "src": _i64(m[1] for m in moves)})
    v = a.views
    _abi.call("rls_copy_rows", ops._ptr(v["xs"]), ops._ptr(v["vs"]), n, ops._ptr(v["dst"]), ops._ptr(v["src"]), len(moves), ops._stream(oc.DEV))
    torch.cuda.synchronize()
    want_x, want_v = _copy_rows_want(xs0, vs0, [m[0] for m in moves], [m[1] for m in moves])
    assert a.bands_intact() and np.array_equal(v["xs"].cpu().numpy(), want_x) and np.array_equal(v["vs"].cpu().numpy(), want_v)


def _message(row, env_id):
    return np.concatenate([np.frombuffer(int(env_id % (1 << 64)).to_bytes(8, "little"), dtype=np.uint8), np.packbits(row, bitorder="little")])


@gpu
@pytest.mark.parametrize("n", [8, 65, 203])
@pytest.mark.parametrize("rows", [1, 7])
def test_winner_message_treats_an_index_outside_its_rows_as_not_mine(n, rows):
    """index[0] is read on the device.  With B > 1 a value outside [0, B) writes zeros -- what a rank without envs writes -- and
    B - 1 packs the last row; with B = 1 the row is the row and the index only supplies the env id."""
    r = oc.rng(n * 10 + rows)
    xs0 = r.randint(0, 2, size=(rows, n)).astype(np.uint8)
    nb, off = 8 + (n + 7) // 8, 1 << 33
    key = _i64([(37 << 20) | 5])
    for idx in (0, rows - 1, -1, rows, I64_MIN):
        for low in (5, 4):                                  # the winning rank, another rank
            a = Arena({"xs": oc.t(xs0).view(torch.bool), "index": _i64([idx]), "key": key, "msg": torch.zeros(nb, dtype=torch.uint8, device=oc.DEV)},
                      fill=("msg",))
            oc.call("winner_message", [a.views["xs"], a.views["index"], a.views["key"], 20, low, off, n, a.views["msg"]])
            torch.cuda.synchronize()
            inside = rows == 1 or 0 <= idx < rows
            want = _message(xs0[idx if rows > 1 else 0], idx + off) if (inside and low == 5) else np.zeros(nb, dtype=np.uint8)
            assert a.bands_intact(), (idx, low)
            assert np.array_equal(a.views["msg"].cpu().numpy(), want), (idx, low)
    if rows == 1:                                           # the single row as a 1-D tensor
        a = Arena({"xs": oc.t(xs0[0]).view(torch.bool), "index": _i64([3]), "key": key, "msg": torch.zeros(nb, dtype=torch.uint8, device=oc.DEV)},
                  fill=("msg",))
        oc.call("winner_message", [a.views["xs"], a.views["index"], a.views["key"], 20, 5, off, n, a.views["msg"]])
        assert a.bands_intact() and np.array_equal(a.views["msg"].cpu().numpy(), _message(xs0[0], 3 + off))


# ---- path_length of the ISCO steps: clamped to [1, N]
def _lengths(n):
    """path_length of 6 samples that share one x and one set of draws, and what each is clamped to"""
    return np.array([0, -3, n, n + 5, 1, n], dtype=np.int64), np.array([1, 1, n, n, 1, n], dtype=np.int64)


def _twins_equal(got, what):
    """samples 0 and 1 (lengths 0, -3) are sample 4 (length 1); samples 2 and 3 (N, N + 5) are sample 5 (N): every output, bit for bit"""
    for part in got:
        bits = part.view(np.uint8).reshape(part.shape[0], -1) if part.dtype != bool else part.reshape(part.shape[0], -1)
        for env, twin in ((0, 4), (1, 4), (2, 5), (3, 5)):
            assert np.array_equal(bits[env], bits[twin]), f"{what}: sample {env} differs from its clamped twin {twin}"


def _one_sample_six_times(r, width):
    x = np.repeat((r.rand(1, width) < 0.5).astype(np.float32), 6, axis=0)
    ug = np.repeat(r.rand(1, width).astype(np.float32).clip(1e-7, 1 - 1e-7), 6, axis=0)
    ua = np.full(6, np.float32(r.rand()), dtype=np.float32)
    return x, ug, ua


def _forced(force_wg):
    from tests.test_gpu_step_store import knobs
    return knobs(RLS_ISCO_FORCE_WG=force_wg)


def _compare_maxcut(got, want, pl, what):
    """_check_maxcut of tests/test_gpu_isco_steps.py on a step already made (its tolerances take the CLAMPED path length)"""
    from tests.isco_tol import RTOL, assert_ll_close, ll_atol
    y, energy, acc, terms, mask = got
    mass, margin = want["remaining_mass"], want["accept_margin"]
    assert np.array_equal(mask.astype(np.uint8), want["mask"].astype(np.uint8)), what
    np.testing.assert_allclose(terms[:, 0], want["ll_x"], rtol=RTOL, atol=1e-5)
    np.testing.assert_allclose(terms[:, 2], want["ll_y"], rtol=RTOL, atol=1e-5)
    np.testing.assert_allclose(energy, want["energy"], rtol=RTOL, atol=1e-5)
    for c, k in ((1, "ll_x2y"), (3, "ll_y2x"), (4, "log_acc")):
        assert_ll_close(terms[:, c], want[k], mass, f"{what}/{k}", pl)
    ok = mass >= 1e-6
    assert bool((np.abs(acc - want["acc"])[ok] <= 2 * ll_atol(mass, pl)[ok]).all()), what
    sure = margin > 2 * (ll_atol(mass, pl) + RTOL * np.abs(want["log_acc"]))
    assert np.array_equal(y[sure], want["y"][sure].astype(np.float32)) and set(np.unique(y)) <= {0.0, 1.0}, what


@gpu
@pytest.mark.parametrize("n,force_wg", [(70, 0), (260, 0), (260, 1)])
def test_isco_maxcut_step_clamps_path_length(n, force_wg):
    from oracle import oracle_isco as oi
    from tests.gpu_util import gnm_arr
    from tests.test_gpu_isco_steps import _maxcut_sampler
    g = gnm_arr(n, 3 * n, 5)
    pl, clamped = _lengths(n)
    x, ug, ua = _one_sample_six_times(oc.rng(n), n)
    s = _maxcut_sampler(g, n, 6)
    with _forced(force_wg):
        got = s.step(oc.t(x), oc.t(pl), 0.7, draws={"u_gumbel": torch.from_numpy(ug), "u_accept": torch.from_numpy(ua)}, want_terms=True)
    got = [o.cpu().numpy() for o in got]
    _twins_equal(got, f"n={n} wg={force_wg}")
    _compare_maxcut(got, oi.maxcut_step(x, g[:, 0], g[:, 1], clamped, 0.7, ug, ua), clamped, f"n={n} wg={force_wg}")


@gpu
@pytest.mark.parametrize("n,force_wg", [(70, 0), (260, 0), (260, 1)])
def test_isco_mis_step_clamps_path_length(n, force_wg):
    from tests import mis_oracle as mo
    from tests.test_gpu_isco_mis import LAM, _check_mis, _sampler, _step
    eu, ev = mo.gnm_multigraph(n, 3 * n, 5)
    pl, clamped = _lengths(n)
    x, ug, ua = _one_sample_six_times(oc.rng(n + 1), n)
    s = _sampler(eu, ev, n, 6, lam=LAM)
    with _forced(force_wg):
        got = _step(s, x, pl, 0.7, ug, ua)
    _twins_equal(got, f"n={n} wg={force_wg}")
    r = mo.mis_step(x, eu, ev, LAM, clamped, 0.7, ug, ua)
    _check_mis(got, x, r, clamped, mo.mask_is_decided(x, eu, ev, LAM, clamped, 0.7, ug), f"n={n} wg={force_wg}")


@gpu
@pytest.mark.parametrize("n,force_wg", [(70, 0), (260, 0), (260, 1)])
def test_pisco_step_clamps_path_length(n, force_wg):
    from tests import pisco_oracle as po
    from tests.test_gpu_pisco import _check_step, _sampler, _step
    adj = po.dense_graph(n, 0.1, 2, n).astype(np.float16)
    Np = adj.shape[0]
    assert Np == po.pad8(n) and Np in (72, 264)
    pl, clamped = _lengths(Np)
    x, ug, ua = _one_sample_six_times(oc.rng(n + 2), Np)
    x = x.astype(np.float16)
    s = _sampler(adj, n, 6)
    with _forced(force_wg):
        got = _step(s, x, pl, 0.7, ug, ua)
    _twins_equal(got, f"Np={Np} wg={force_wg}")
    r = po.step(x, adj, clamped, 0.7, ug, ua)
    _check_step(got, x, r, clamped, po.mask_is_decided(x, adj, clamped, 0.7, ug), f"Np={Np} wg={force_wg}", po.K_TOL)


# ---- ids of rls_s2vppo_reset: an id outside [0, num_envs) is skipped
@gpu
@pytest.mark.parametrize("form", ["wave", "workgroup"])
def test_s2vppo_reset_skips_ids_outside_the_batch(form):
    from tests.test_gpu_s2v_ppo import _thresholds
    wave = _thresholds()[0]
    sizes = (9, 30, wave if form == "wave" else wave + 1, 17, 65)
    env = oc.s2v_env(sizes)
    assert env.launch_plan()["form"] == form
    r = oc.rng(wave)
    env.reset(z0=r.choice(np.array([-1, 1], dtype=np.int8), size=sum(sizes)))
    for _ in range(3):                                       # a state a reset has something to undo in
        env.step(torch.tensor([int(r.randint(0, n)) for n in sizes], dtype=torch.int64, device=oc.DEV))
    z1 = r.choice(np.array([-1, 1], dtype=np.int8), size=sum(sizes))
    args = oc.taken("s2vppo_reset", lambda: env.reset(ids=[1, 3], z0=z1))
    nm = oc.names("s2vppo_reset")
    a = Arena({n: v for n, v in zip(nm, args) if isinstance(v, torch.Tensor)})
    base = [a.views.get(n, v) if isinstance(v, torch.Tensor) else v for n, v in zip(nm, args)]
    before = a.buf.clone()
    oc.call("s2vppo_reset", base)                            # the named envs alone, in order
    torch.cuda.synchronize()
    want = a.buf.clone()
    assert a.bands_intact() and not torch.equal(want, before)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    keep = np.ones(sum(sizes), dtype=bool)
    for e in (1, 3):
        keep[ptr[e]:ptr[e + 1]] = False
        assert np.array_equal(a.views["z"].cpu().numpy()[ptr[e]:ptr[e + 1]], z1[ptr[e]:ptr[e + 1]])
    moved = Arena({n: v for n, v in zip(nm, args) if isinstance(v, torch.Tensor)})        # the same layout: the state before the reset
    for n in ("z", "delta", "last_flip", "best_z", "mask", "x"):
        assert np.array_equal(a.views[n].cpu().numpy()[keep], moved.views[n].cpu().numpy()[keep]), n
    for n in ("counters", "cut", "best_cut", "tabu", "hash"):
        rows = [0, 2, 4]
        assert torch.equal(a.views[n][rows], moved.views[n][rows]), n
    for ids in ([-1, len(sizes), 3, 1], [3, I64_MIN, 1, -1], [len(sizes), 1, 3]):
        a.buf.copy_(before)
        with_ids = Arena({"ids": _i64(ids)})
        base[nm.index("ids")] = with_ids.views["ids"]
        oc.call("s2vppo_reset", base)
        torch.cuda.synchronize()
        assert with_ids.bands_intact() and torch.equal(a.buf, want), ids


# ---- the actions of the three steps: the ends of int64 beside -1 and N
@gpu
def test_maxcut_step_leaves_an_env_whose_action_is_at_the_ends_of_int64():
    g, n = oc.graph(), oc.N
    xs = oc.spins(rows=6)
    obj0 = oc.cut_of(xs)
    acts = [3, I64_MAX, I64_MIN, -1, n, n - 1]
    a = Arena({"x_in": xs, "x_out": xs.clone(), "action": _i64(acts), "obj": obj0.to(torch.int32), "reward": torch.zeros(6, device=oc.DEV)},
              fill=("reward",))
    v = a.views
    oc.call("maxcut_step", [g.handle, v["x_in"], v["x_out"], v["action"], v["obj"], v["reward"], None, None, 0.0])
    torch.cuda.synchronize()
    x0, x1 = xs.cpu().numpy(), v["x_out"].cpu().numpy()
    want = x0.copy()
    want[0, 3] ^= True
    want[5, n - 1] ^= True
    obj1 = oc.cut_of(oc.t(want)).cpu().numpy()
    rew = v["reward"].cpu().numpy()
    assert a.bands_intact() and np.array_equal(x1, want) and np.array_equal(v["x_in"].cpu().numpy(), x0)
    assert np.isnan(rew[1:5]).all() and np.array_equal(rew[[0, 5]], (obj1 - obj0.cpu().numpy())[[0, 5]].astype(np.float32))
    assert np.array_equal(v["obj"].cpu().numpy(), obj1.astype(np.int32))


@gpu
def test_spin_step_leaves_an_env_whose_action_is_at_the_ends_of_int64():
    from rlsolver_amd.envs.spinsystem import S2V_OBSERVABLES, SpinSystem
    from rlsolver_amd.graph import generate_gnm
    env = SpinSystem(generate_gnm(40, 90, 1), 40, 4, max_steps=5, observables=S2V_OBSERVABLES, device=oc.DEV, include_adjacency=False)
    before, score = env.state.clone(), env.score.clone()
    _, r, _ = env.step(_i64([3, I64_MAX, I64_MIN, 39]))
    assert bool(torch.isnan(r[1])) and bool(torch.isnan(r[2])) and not bool(torch.isnan(r[0])) and not bool(torch.isnan(r[3]))
    assert torch.equal(env.state[1:3], before[1:3]) and torch.equal(env.score[1:3], score[1:3])
    assert not torch.equal(env.state[0], before[0]) and not torch.equal(env.state[3], before[3])


@gpu
def test_s2vppo_step_leaves_an_env_whose_action_is_at_the_ends_of_int64():
    from tests.s2vppo_checks import bits, snap_env
    env = oc.s2v_env((20, 20, 20))
    before = snap_env(env)
    env.step(_i64([I64_MAX, I64_MIN, 7]))
    after = snap_env(env)
    assert np.isnan(after["reward"][:2]).all() and not np.isnan(after["reward"][2]) and not after["done"].any()
    for key in ("z", "delta", "best_z", "mask"):
        assert np.array_equal(bits(before[key])[:40], bits(after[key])[:40]), key
        assert not np.array_equal(bits(before["z"])[40:], bits(after["z"])[40:])
    for key in ("cut", "best", "steps"):
        assert np.array_equal(bits(before[key])[:2], bits(after[key])[:2]), key
    assert after["steps"][2] == 1
