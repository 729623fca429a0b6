"""Numpy restatement of the MaxSAT family of the upstream MCPG package: loader, metro walk, node-sequential sweep and
score (rlsolver/methods/MCPG/dataloader.py:163-275, sampling.py:67-86, 253-285), written from their description.  The
sweep evaluates the reference's float32 accept expression on the recorded uniforms; every sum is a float32 sum of
integers (exact below 2^24, in any order).  Tests compare the HIP path against this; tests/golden/maxsat.npz ties it
to the reference itself."""
import numpy as np

F = np.float32


class Instance:
    """What the loader leaves: the global literal lists and, per variable, the concatenated literal lists of every
    clause that holds it -- once per OCCURRENCE of the variable -- with fresh local clause ids."""

    def __init__(self, nvar, clauses, weights=None, top=None, nclause=None):
        self.nvar, self.clauses = int(nvar), [list(map(int, c)) for c in clauses]
        self.weights = None if weights is None else [int(w) for w in weights]
        self.top = None if weights is None else int(top)
        self.nclause = len(self.clauses) if nclause is None else int(nclause)
        self.nhard = 0 if weights is None else sum(1 for w in self.weights if w == self.top)
        vi, ci, neg = [], [], []
        self.nvi, self.nci, self.nneg = ([[] for _ in range(self.nvar)] for _ in range(3))
        self.degree = np.zeros(self.nvar, dtype=np.float32)
        for c, cl in enumerate(self.clauses):
            w = 1 if weights is None else self.weights[c]
            tvi = [abs(l) - 1 for l in cl]
            tneg = [(1 if l > 0 else -1) * w for l in cl]
            vi += tvi
            ci += [c] * len(cl)
            neg += tneg
            for v in tvi:
                self.degree[v] += 1
                self.nvi[v] += tvi
                self.nneg[v] += tneg
                nxt = self.nci[v][-1] + 1 if self.nci[v] else 0
                self.nci[v] += [nxt] * len(cl)
        self.vi, self.ci, self.neg = (np.asarray(a, dtype=np.int64) for a in (vi, ci, neg))
        self.K = self.nclause if weights is None else self.nclause - self.nhard + self.top * self.nhard


def parse(text, ext):
    """The loader's reading of a .cnf / .wcnf text: one clause per line; .cnf drops every token "0", .wcnf takes the
    first token as the weight and drops the last one; the header's fifth field is the hard weight."""
    nvar = nclause = top = None
    clauses, weights = [], []
    for line in text.splitlines():
        t = line.split()
        if not t or t[0] == "c":
            continue
        if t[0] == "p":
            nvar, nclause = int(t[2]), int(t[3])
            if ext == ".wcnf":
                top = int(t[4])
            continue
        if ext == ".wcnf":
            weights.append(int(t[0]))
            clauses.append([int(x) for x in t[1:-1]])
        else:
            clauses.append([int(x) for x in t if x != "0"])
    return Instance(nvar, clauses, weights if ext == ".wcnf" else None, top, nclause)


def _segment_max_sum(cal, seg):
    """sum over segments of the per-segment maximum (scatter reduce="max", then sum); cal [C, L], seg [L]."""
    if cal.shape[1] == 0:
        return np.zeros(cal.shape[0], dtype=F)
    n = int(seg.max()) + 1
    out = np.full((cal.shape[0], n), -np.inf, dtype=F)
    np.maximum.at(out, (slice(None), seg), cal)
    out[:, np.isinf(out[0])] = 0            # a clause id without a literal (an empty clause) contributes 0
    return out.sum(axis=1, dtype=F)


def metro(probs, start, T, index, u):
    """The walk: up to 5 T rounds, stopping before the first round at which the accept count has reached C * T."""
    x = start.astype(bool).copy()
    C = x.shape[1]
    cols = np.arange(C)
    probs = probs.astype(F)
    count = 0
    for t in range(min(5 * T, index.shape[0])):
        if count >= C * T:
            break
        i = index[t]
        val = x[i, cols]
        p = np.where(val, probs[i], F(1) - probs[i]).astype(F)
        acc = u[t].astype(F) < (F(1) - p) / p
        x[i, cols] = np.where(acc, ~val, val)
        count += int(acc.sum())
    return x.astype(F)


def accept(new, old, u):
    """The reference's float32 rule: new > (old + u) - 0.5, each operation rounded to float32."""
    return new.astype(F) > ((old.astype(F) + u.astype(F)).astype(F) - F(0.5)).astype(F)


def visit(inst, s, order, num_ls, decide):
    """The node-sequential sweep with the accept rule left to the caller.  s float32 [C, nvar] of -1 | +1, in place.  For every
    pass and visiting position: old = the listed sum of variable i, new = the same with s_i negated, and
    decide(cnt, pos, i, old, new) -> bool [C] says in which chains the flip is kept (s[:, i] holds the FLIPPED value when it is
    called).  sweep, coin_rule_agrees and the tests that follow the kernel through its ties are this one loop."""
    for cnt in range(num_ls):
        for pos in range(inst.nvar):
            i = int(order[pos])
            idx, seg = np.asarray(inst.nvi[i], dtype=np.int64), np.asarray(inst.nci[i], dtype=np.int64)
            ng = np.asarray(inst.nneg[i], dtype=F)
            old = _segment_max_sum(s[:, idx] * ng, seg)
            s[:, i] = -s[:, i]
            new = _segment_max_sum(s[:, idx] * ng, seg)
            keep = decide(cnt, pos, i, old, new)
            s[:, i] = np.where(keep, s[:, i], -s[:, i])
    return s


def sweep(inst, s, order, num_ls, uniforms):
    """s float32 [C, nvar] of -1 | +1, in place; uniforms [num_ls, nvar (visiting position), C]."""
    return visit(inst, s, order, num_ls, lambda cnt, pos, i, old, new: accept(new, old, uniforms[cnt, pos]))


def score(inst, s):
    """S float32 [C] = sum over clauses of max_lit(s_v neg)."""
    return _segment_max_sum(s[:, inst.vi] * inst.neg.astype(F), inst.ci)


def result(inst, s):
    """res = (S + K) / 2 in float32."""
    return ((score(inst, s) + F(inst.K)).astype(F) / F(2)).astype(F)


def sampling(inst, order, start, probs, num_ls, change_times, M, index, u, uniforms):
    """mcpg_sampling_maxsat's four returns: (max_res [M], best 0|1 [nvar, M], raw [nvar, C], -(res - mean(res)) [C]),
    and the chains after the sweep 0|1 [nvar, C] and S [C] besides."""
    raw = metro(probs, start, change_times, index, u)
    s = (raw.T * F(2) - F(1)).astype(F).copy()
    sweep(inst, s, order, num_ls, uniforms)
    S = score(inst, s)
    res = ((S + F(inst.K)).astype(F) / F(2)).astype(F)
    C = res.shape[0]
    best = np.argmax(res.reshape(-1, M), axis=0) * M + np.arange(M)
    x = ((s + F(1)) / F(2)).astype(F)
    mean = (res.sum(dtype=F) / F(C)).astype(F)
    return res[best], x.T[:, best], raw, -(res - mean), x.T.copy(), S


def coin_rule_agrees(inst, s, order, num_ls, uniforms):
    """True when, on this run, the float32 rule equals  d > 0 or (d == 0 and u < 1/2)  at every decision (what the
    kernel computes from coins): replays the sweep with both."""
    agree = [True]

    def decide(cnt, pos, i, old, new):
        keep = accept(new, old, uniforms[cnt, pos])
        d = new.astype(np.float64) - old.astype(np.float64)
        agree[0] = agree[0] and np.array_equal(keep, (d > 0) | ((d == 0) & (uniforms[cnt, pos] < F(0.5))))
        return keep
    visit(inst, s.copy(), order, num_ls, decide)
    return agree[0]


def prepare_uniforms(u):
    """Recorded uniforms as the GPU tests use them: a draw in the band 0 < 1/2 - u <= 2^-10, where the float32 rule may
    drop a tie the coin keeps, becomes 0.25."""
    u = np.asarray(u, dtype=F).copy()
    band = (F(0.5) - u > 0) & (F(0.5) - u <= F(2.0 ** -10))
    u[band] = F(0.25)
    return u


def replay_schedule(lv_ptr, lv_data, nvar, words, num_ls, coins):
    """The level schedule of rls_maxsat_visit_levels (include/rlsolver_hip.h) decoded in plain Python: the variables of a
    level are all decided from the state BEFORE the level.  words: python ints (64 chains each) [nvar]; coins[cnt][pos]: the
    tie word.  Returns the words after num_ls passes."""
    full = (1 << 64) - 1
    lp = np.asarray(lv_ptr).view(np.uint32).astype(np.int64)
    data = np.asarray(lv_data).view(np.uint32).astype(np.int64)
    G = lp.size - 1
    x = list(words) + [0]
    for cnt in range(num_ls):
        pre = None
        for k in range(G):
            if lp[k] >> 31 or pre is None:
                pre = list(x)                                  # a level boundary: later groups read this state
            weighted, B = (lp[k] >> 30) & 1, 512 if (lp[k] >> 30) & 1 else 256
            p0, p1 = (lp[k] & 0xFFFFFF) * 64, (lp[k + 1] & 0xFFFFFF) * 64
            blocks = (p1 - p0 - 128) // B
            assert (p1 - p0 - 128) % B == 0
            for lane in range(64):
                var, pos = int(data[p0 + 2 * lane]), int(data[p0 + 2 * lane + 1])
                if var >= nvar:
                    continue
                make = brk = 0
                mk = [0] * 64
                others, xi = 0, pre[var]
                for r in range(4 * blocks):
                    at = p0 + 128 + (r // 4) * B + 4 * lane + r % 4
                    e = int(data[at])
                    v = (e & 0x3FFF8) >> 3
                    assert v <= nvar
                    others |= pre[v] ^ (full if e >> 31 else 0)
                    if e & 1:
                        cls, w = (e >> 1) & 3, int(data[at + 256]) if weighted else 1
                        crit = 0 if cls == 3 else (~others & full)
                        own = xi ^ (full if cls == 2 else 0)
                        for c in range(64):
                            if (crit >> c) & 1:
                                mk[c] += w if not (own >> c) & 1 else -w
                        others = 0
                planes = (lp[k] >> 24) & 31
                flip = 0
                for c in range(64):
                    assert abs(mk[c]) < (1 << planes)
                    if mk[c] > 0 or (mk[c] == 0 and (coins[cnt][pos] >> c) & 1):
                        flip |= 1 << c
                x[var] = xi ^ flip
    return x[:nvar]
