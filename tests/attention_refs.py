"""Float64 references, a seeded case generator and guarded device buffers for the geometry tests of the attention cores
(tests/test_hip_attention_geometry.py; the references and the generator are checked on the CPU by
tests/test_attention_refs_cpu.py).  A plain module: nothing here is collected by pytest and nothing touches the GPU on import.

Shapes.  q, dout, out and dq are [b, heads, tq, d]; k, v, dk and dv are [b, hk, tk, d] with hk = heads, or hk = 1 for multi-query
sharing (one K / V for all heads: the references broadcast it, and autograd sums dk / dv over the heads).  A key mask is a
bool [b, tk], True = attend.
"""
import random

import torch

# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------


def ref_attention(q, k, v, scale, mask=None):
    """softmax(scale q k^T) v in float64 -> (out [b, heads, tq, d], lse [b, heads, tq]: log-sum-exp of the scaled logits over
    the attended keys).  A masked key has weight exactly 0 and is absent from lse."""
    q, k, v = q.double(), k.double(), v.double()
    s = torch.einsum("bhid,bhjd->bhij", q, k.expand(-1, q.shape[1], -1, -1)) * scale
    if mask is not None:
        s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
    lse = torch.logsumexp(s, -1)
    out = torch.einsum("bhij,bhjd->bhid", torch.exp(s - lse[..., None]), v.expand(-1, q.shape[1], -1, -1))
    return out, lse


def ref_attention_grads(q, k, v, dout, scale, mask=None):
    """(dq, dk, dv) of sum(out * dout) through torch.autograd in float64; dk / dv have k's shape (multi-query: head sums)"""
    q, k, v = (t.double().detach().clone().requires_grad_(True) for t in (q, k, v))
    out, _ = ref_attention(q, k, v, scale, mask)
    (out * dout.double()).sum().backward()
    return q.grad, k.grad, v.grad


def ref_attention_grad_scales(q, k, v, dout, scale, mask=None):
    """The absolute-value form of each gradient, (dq~, dk~, dv~) in float64, shaped like (dq, dk, dv):
        dq~ = scale A |k|,  dk~ = scale A^T |q|,  dv~ = P^T |dout|,   A = P (|dP| + |D|),  dP = dout v^T,  D = dout . out
    -- the same sums as dq, dk, dv with every term taken positive, so |dq| <= dq~ element by element (likewise dk, dv) and
    any evaluation in floating point carries rounding errors in units of them.  They stand in for a gradient's own maximum
    where that is exactly zero: a row that attends to one key alone (tk == 1, a mask that leaves key 0 only) has P = 1 and
    dP = D, hence dS = 0 and dq = dk = 0, while a kernel returns the rounding of dP - D."""
    q, k, v, dout = q.double(), k.double(), v.double(), dout.double()
    heads = q.shape[1]
    out, lse = ref_attention(q, k, v, scale, mask)
    ke, ve = k.expand(-1, heads, -1, -1), v.expand(-1, heads, -1, -1)
    s = torch.einsum("bhid,bhjd->bhij", q, ke) * scale
    if mask is not None:
        s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
    p = torch.exp(s - lse[..., None])
    a = p * (torch.einsum("bhid,bhjd->bhij", dout, ve).abs() + (dout * out).sum(-1).abs()[..., None])
    dq = scale * torch.einsum("bhij,bhjd->bhid", a, ke.abs())
    dk = scale * torch.einsum("bhij,bhid->bhjd", a, q.abs())
    dv = torch.einsum("bhij,bhid->bhjd", p, dout.abs())
    if k.shape[1] == 1:
        dk, dv = dk.sum(1, keepdim=True), dv.sum(1, keepdim=True)
    return dq, dk, dv


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
BATCHES = (1, 2)
HEADS = (1, 2, 3)
# one lane, the 32-query wave boundary, the 128-query block boundary, a ragged last block
TQS = (1, 31, 32, 33, 127, 128, 129, 200, 257)
# below a sub-tile, the 32- and 64-key tile boundaries (both key-tile sizes), odd tails for the pairwise V staging, the shipped 273
TKS = (1, 2, 31, 32, 33, 63, 64, 65, 97, 273)
LAYOUTS = ("legacy", "separate", "mq")
PADS = (0, 4, 12)
SHARPS = (1, 4)
MASK_PATTERNS = ("random", "only_key0", "last_masked", "subtile_then_valid", "valid_then_subtile")
PAD_KEYS = ("q_pad", "kv_pad", "out_pad", "dout_pad")


def _pattern_fits(pattern, tk):
    if pattern == "last_masked":
        return tk >= 2
    if pattern == "subtile_then_valid":          # keys [32, 64) masked, key 64 valid
        return tk >= 65
    if pattern == "valid_then_subtile":          # the last (possibly partial) 32-key sub-tile masked, the key before it valid
        return tk >= 33
    return True


def _spread(rnd, values, count):
    """`count` draws from `values` in which every value appears (count >= len(values)), in random order"""
    assert count >= len(values), (count, values)
    out = list(values) + [rnd.choice(values) for _ in range(count - len(values))]
    rnd.shuffle(out)
    return out


def attention_cases(n, seed, *, dims, masked, backward=False):
    """`n` dicts, each describing one launch completely (its data come from case["seed"]).  Seeded and stratified: every value
    of BATCHES, HEADS, dims, TQS, TKS, SHARPS, of the layouts in use and of PADS for each of the four strides -- and, masked, of
    MASK_PATTERNS -- appears in at least one case (stratification_gaps() lists what does not).

    layout "legacy":   one fused [b, t, 3 heads d (+ pad)] buffer, head h at +3 h d, k at +d, v at +2d; q_ld == kv_ld and
                       tq == tk = t, drawn from TQS and TKS together (TQS and TKS are covered by the other layouts alone)
           "separate": q [b, tq, heads d (+ pad)] and [k | v] [b, tk, 2 heads d (+ pad)], kv_hs = d
           "mq":       q as above and one [k | v] [b, tk, 2 d (+ pad)] for all heads, kv_hs = 0
    masked: "separate" and "mq" only; backward (with masked): the masked backward takes kv_hs = 0 only with one head, so "mq"
    cases have heads = 1 and HEADS is covered by the "separate" cases."""
    rnd = random.Random(seed)
    layouts = LAYOUTS[1:] if masked else LAYOUTS
    lay = [layouts[i % len(layouts)] for i in range(n)]          # the layouts in equal shares
    rnd.shuffle(lay)
    free = [i for i in range(n) if lay[i] != "legacy"]           # cases whose tq, tk and kv_ld are drawn on their own
    cases = [dict(layout=lay[i]) for i in range(n)]
    for key, values in (("b", BATCHES), ("d", tuple(dims)), ("sharp", SHARPS), ("q_pad", PADS), ("out_pad", PADS),
                        ("dout_pad", PADS)):
        for cs, val in zip(cases, _spread(rnd, values, n)):
            cs[key] = val
    for i, val in zip(free, _spread(rnd, PADS, len(free))):
        cases[i]["kv_pad"] = val
    one_head = [i for i in range(n) if masked and backward and lay[i] == "mq"]
    many = [i for i in range(n) if i not in one_head]
    for i, val in zip(many, _spread(rnd, HEADS, len(many))):
        cases[i]["heads"] = val
    for i in one_head:
        cases[i]["heads"] = 1
    for i, val in zip(free, _spread(rnd, TQS, len(free))):
        cases[i]["tq"] = val
    for i, val in zip(free, _spread(rnd, TKS, len(free))):
        cases[i]["tk"] = val
    both = tuple(sorted(set(TQS) | set(TKS)))
    for i in range(n):
        if lay[i] == "legacy":
            cases[i]["tq"] = cases[i]["tk"] = rnd.choice(both)
    if masked:
        todo = list(reversed(MASK_PATTERNS))                     # the patterns that need the most keys first
        order = list(range(n))
        rnd.shuffle(order)
        for i in order:                                          # every pattern once, on a case whose tk can hold it ...
            fits = [p for p in todo if _pattern_fits(p, cases[i]["tk"])]
            if fits:
                cases[i]["mask_pattern"] = fits[0]
                todo.remove(fits[0])
        assert not todo, todo
        for cs in cases:                                         # ... the others at random among those that fit
            if "mask_pattern" not in cs:
                cs["mask_pattern"] = rnd.choice([p for p in MASK_PATTERNS if _pattern_fits(p, cs["tk"])])
    for cs in cases:
        b, heads, d = cs["b"], cs["heads"], cs["d"]
        if cs["layout"] == "legacy":
            cs["kv_pad"] = cs["q_pad"]                           # one buffer, one row stride
            cs["q_ld"] = cs["kv_ld"] = 3 * heads * d + cs["q_pad"]
            cs["q_hs"] = cs["kv_hs"] = 3 * d
        else:
            cs["q_ld"], cs["q_hs"] = heads * d + cs["q_pad"], d
            if cs["layout"] == "separate":
                cs["kv_ld"], cs["kv_hs"] = 2 * heads * d + cs["kv_pad"], d
            else:
                cs["kv_ld"], cs["kv_hs"] = 2 * d + cs["kv_pad"], 0
        cs["out_ld"] = heads * d + cs["out_pad"]                 # forward: o_ld is out_ld
        cs["dout_ld"] = heads * d + cs["dout_pad"]
        cs["masked"] = bool(masked)
        cs["seed"] = rnd.randrange(1 << 30)
    return cases


# the sweeps of tests/test_hip_attention_geometry.py: the generator's CPU test checks the promise for exactly these draws
SWEEPS = {
    "plain": dict(n=24, seed=20261019, dims=(16, 32, 64, 128), masked=False),          # forward (both cores), exact backward
    "plain_to_64": dict(n=24, seed=20261020, dims=(16, 32, 64), masked=False),         # split backward (no 128-wide instance)
    "masked": dict(n=24, seed=20261021, dims=(16, 32, 64, 128), masked=True),
    "masked_backward": dict(n=24, seed=20261022, dims=(16, 32, 64, 128), masked=True, backward=True),
}


def sweep_cases(name):
    kw = dict(SWEEPS[name])
    return attention_cases(kw.pop("n"), kw.pop("seed"), **kw)


def stratification_gaps(cases, *, dims, masked):
    """[(key, value)] of every promised value that no case carries ([] = the promise of attention_cases is kept)"""
    want = dict(b=BATCHES, heads=HEADS, d=tuple(dims), tq=TQS, tk=TKS, sharp=SHARPS, layout=LAYOUTS[1:] if masked else LAYOUTS)
    want.update({k: PADS for k in PAD_KEYS})
    if masked:
        want["mask_pattern"] = MASK_PATTERNS
    return [(key, val) for key, values in want.items() for val in values if not any(cs[key] == val for cs in cases)]


def case_mask(cs):
    """the key mask of a masked case, bool [b, tk] (True = attend), or None.  Key 0 is always valid; each batch row draws its
    own random part."""
    if not cs["masked"]:
        return None
    g = torch.Generator().manual_seed(cs["seed"] ^ 0x5A5A)
    b, tk, pattern = cs["b"], cs["tk"], cs["mask_pattern"]
    mask = torch.rand(b, tk, generator=g) > 0.4
    if pattern == "only_key0":
        mask[:] = False
    elif pattern == "last_masked":
        mask[:, -1] = False
    elif pattern == "subtile_then_valid":
        mask[:, 32:64] = False
        mask[:, 64] = True
    elif pattern == "valid_then_subtile":
        first = (tk - 1) // 32 * 32
        mask[:, first:] = False
        mask[:, first - 1] = True
    mask[:, 0] = True
    return mask


def case_tensors(cs):
    """fp32 CPU inputs of a case: q (times the case's logit sharpness), k, v, dout in the shapes of the module docstring, the
    softmax scale d^-0.5 and the mask"""
    g = torch.Generator().manual_seed(cs["seed"])
    b, heads, d, tq, tk = cs["b"], cs["heads"], cs["d"], cs["tq"], cs["tk"]
    hk = 1 if cs["layout"] == "mq" else heads
    q = torch.randn(b, heads, tq, d, generator=g) * float(cs["sharp"])
    k = torch.randn(b, hk, tk, d, generator=g)
    v = torch.randn(b, hk, tk, d, generator=g)
    dout = torch.randn(b, heads, tq, d, generator=g)
    return dict(q=q, k=k, v=v, dout=dout, scale=d ** -0.5, mask=case_mask(cs))


def rows_of(t, ld):
    """[b, h, n, d] -> the row layout of the entry points, [b, n, ld] with head h at columns [h d, (h + 1) d) and NaN in the
    padding columns (an input's padding must never be read: a NaN there would reach the result)"""
    b, h, n, d = t.shape
    out = torch.full((b, n, ld), float("nan"), dtype=t.dtype)
    out[:, :, :h * d] = t.permute(0, 2, 1, 3).reshape(b, n, h * d)
    return out


def heads_of(rows, h, d):
    """inverse of rows_of on the first h d columns: [b, n, >= h d] -> [b, h, n, d]"""
    b, n, _ = rows.shape
    return rows[:, :, :h * d].reshape(b, n, h, d).permute(0, 2, 1, 3)


def legacy_rows(q, k, v, ld):
    """the fused legacy buffer [b, t, ld]: head h holds [q | k | v] at columns [3 h d, 3 (h + 1) d), NaN padding"""
    b, h, t, d = q.shape
    out = torch.full((b, t, ld), float("nan"), dtype=q.dtype)
    out[:, :, :3 * h * d] = torch.stack([q, k, v], 2).permute(0, 3, 1, 2, 4).reshape(b, t, 3 * h * d)
    return out


def legacy_split(rows, h, d):
    """inverse of legacy_rows: [b, t, >= 3 h d] -> (q, k, v), each [b, h, t, d]"""
    b, t, _ = rows.shape
    x = rows[:, :, :3 * h * d].reshape(b, t, h, 3, d).permute(3, 0, 2, 1, 4)
    return x[0], x[1], x[2]


# ---------------------------------------------------------------------------------------------------------------------
# guarded device buffers
# ---------------------------------------------------------------------------------------------------------------------
GUARD_BITS = 0x7FC5A5A5          # a quiet NaN no arithmetic produces


class Guarded:
    """A device output of `rows` rows with row stride `ld` floats of which the kernel owns columns [0, cols), allocated with
    one guard row in front and one behind and prefilled, guards, padding and owned region alike, with GUARD_BITS.  After
    the launch owned() is the owned region (CPU, [rows, cols]) and untouched() says whether every byte outside it still
    holds the pattern (compared as int32: NaN != NaN as floats)."""

    def __init__(self, rows, ld, cols=None, device="cuda"):
        self.rows, self.ld, self.cols = rows, ld, ld if cols is None else cols
        assert 0 < self.cols <= ld
        self.bits = torch.full(((rows + 2) * ld,), GUARD_BITS, dtype=torch.int32, device=device)

    @property
    def ptr(self):
        """address of row 0, column 0 (the guard row in front ends here)"""
        return self.bits.data_ptr() + 4 * self.ld

    def tensor(self):
        """the rows with their padding, a float32 view [rows, ld] on the device"""
        return self.bits.view(torch.float32)[self.ld:(self.rows + 1) * self.ld].view(self.rows, self.ld)

    def owned(self):
        return self.tensor()[:, :self.cols].cpu()

    def untouched(self):
        bits = self.bits.cpu().view(self.rows + 2, self.ld)
        ok = bool((bits[0] == GUARD_BITS).all()) and bool((bits[-1] == GUARD_BITS).all())
        return ok and bool((bits[1:-1, self.cols:] == GUARD_BITS).all())

    def written(self):
        """no element of the owned region still holds the pattern"""
        bits = self.bits.cpu().view(self.rows + 2, self.ld)
        return not bool((bits[1:-1, :self.cols] == GUARD_BITS).any())
