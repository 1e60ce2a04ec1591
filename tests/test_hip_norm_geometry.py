"""The GroupNorm / LayerNorm kernels over seeded random geometry, against float64 (tests/norm_refs.py): channel counts on both
branches of the statistics kernel, row counts around its 32 row lanes, part counts on every tail of the partial fold, the
backward chain through every resample-mode pair with concatenated sources, padded strides, dropout and accumulation, LayerNorm
rows with a ragged last lane group, exactly constant groups, inputs far from zero mean -- and, around every output, guard rows
and padding columns that must come back untouched.  One sweep = one test of 24 to 30 launches or chains, as
tests/test_hip_attention_geometry.py does for the attention cores; tools/norm_geometry_errors.py prints the measured errors
(profiles/norm_geometry_errors.txt)."""
import ctypes as C

import pytest
import torch

import norm_refs as R
from conftest import max_rel

pytestmark = pytest.mark.gpu

TOL = R.TOL
EPS = R.EPS
# "to fp32 rounding".  The coefficient kernels form gamma * rstd * (1 + scale) in double from the float inputs and round to float
# ONCE (at most 2^-24 relative), and `want` below is the same double chain: 2^-23 is twice what a correct kernel can be off by,
# with or without FiLM.  For LayerNorm's rstd it is an rsqrtf of one-ulp accuracy.
ULP = 2.0 ** -23
# offset family, r >= 16: error of a x + b allowed in units of the a-priori bound of rstd's relative error (norm_refs.offset_bound,
# evaluated at the data's own largest group r).  A margin of 4 was set aside for the per-lane fp32 partial sums of
# chan_stats_kernel; measured on the MI355X the error never reaches the bound itself -- the largest error / bound over the six
# (r, hw) cells with r >= 16 is 0.47 (profiles/norm_geometry_errors.txt) -- so the margin is 2 x that ratio
OFFSET_MARGIN = 0.94


def _lib():
    from sgdm_amd import _lib as L
    return L, L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    if t is None:
        return None
    return C.c_void_p(t if isinstance(t, int) else t.data_ptr())


def _raise(failures):
    """every failing case with its index, findings and whole dict (raised by hand: pytest shortens a rewritten assert's message)"""
    if failures:
        raise AssertionError("\n".join(f"case {ci}: {bad}\n    {cs}" for ci, cs, bad in failures))


def _guards(bad, **bufs):
    for nm, buf in bufs.items():
        if buf is None:
            continue
        if not buf.written():
            bad.append(f"an owned element of {nm} was not written")
        if not buf.untouched():
            bad.append(f"a write outside the rows and columns of {nm}")
        if not torch.isfinite(buf.owned()).all():
            bad.append(f"{nm} is not finite")


def _over(bad, worst, nm, err, tol):
    worst[nm] = (max(worst.get(nm, (0.0, tol))[0], err), tol)        # {quantity: (worst error, its tolerance)}
    if not err < tol:
        bad.append((nm, err, tol))


# ---------------------------------------------------------------------------------------------------------------------
# A. sgd_chan_stats
# ---------------------------------------------------------------------------------------------------------------------
def run_chan_stats_sweep(report=None):
    L, lib = _lib()
    worst, failures = {}, []
    for ci, (cs, t, ref, _) in enumerate(R.sweep_reference("chan_stats")):
        n, hw, c, ct, off = cs["n"], cs["hw"], cs["c"], cs["c_total"], cs["c_off"]
        xd = t["x"].cuda()
        sums = R.Guarded(n, 2 * ct, 2 * c, 2 * off)
        L.check(lib.sgd_chan_stats(_p(xd), n, hw, c, _p(sums.ptr), ct, off, _stream()), f"chan_stats case {ci}: {cs}")
        torch.cuda.synchronize()
        got = sums.owned().view(n, c, 2)
        bad, errs = [], {}
        for k, nm in enumerate(("sum", "sumsq")):
            errs[nm] = max_rel(got[..., k], ref["sums"][..., k])
            _over(bad, worst, nm, errs[nm], TOL["sums"])
        _guards(bad, sums=sums)
        if report is not None:
            report.append(f"chan_stats case {ci:2d} n {n} hw {hw:4d} c {c:3d} c_off {off} sum {errs['sum']:.2e} sumsq {errs['sumsq']:.2e}")
        if bad:
            failures.append((ci, cs, bad))
    return worst, failures


# ---------------------------------------------------------------------------------------------------------------------
# B. sgd_stats_reduce / sgd_gn_coef_parts
# ---------------------------------------------------------------------------------------------------------------------
def run_parts_sweep(report=None):
    L, lib = _lib()
    worst, failures = {}, []
    st = _stream()
    for ci, (cs, t, ref, _) in enumerate(R.sweep_reference("parts")):
        n, c0, c1, parts0, parts1, hw, groups = cs["n"], cs["c0"], cs["c1"], cs["parts0"], cs["parts1"], cs["hw"], cs["groups"]
        c, tag = c0 + c1, f"parts case {ci}: {cs}"
        p0 = t["p0"].cuda()
        p1 = t["p1"].cuda() if t["p1"] is not None else None
        x1 = t["x1"].cuda() if t["x1"] is not None else None
        gamma, beta = t["gamma"].cuda(), t["beta"].cuda()
        film = R.padded(t["film"][:, :2 * c], cs["film_ld"]).cuda() if cs["film"] else None
        tables = []
        for _ in range(2):               # the one-launch route's table and the two-launch route's
            s = R.Guarded(n, 2 * c)
            if x1 is not None:           # this source's sums are in place before the fold, written by sgd_chan_stats
                L.check(lib.sgd_chan_stats(_p(x1), n, hw, c1, _p(s.ptr), c, c0, st), "chan_stats " + tag)
            tables.append(s)
        sums, s2 = tables
        torch.cuda.synchronize()
        before = sums.tensor().view(torch.int32)[:, 2 * c0:].clone()
        a, b, a2, b2 = (R.Guarded(n, c) for _ in range(4))
        L.check(lib.sgd_gn_coef_parts(_p(p0), parts0, c0, _p(p1), parts1, c1, _p(sums.ptr), _p(gamma), _p(beta), _p(film),
                                      cs["film_ld"], n, groups, hw, EPS, _p(a.ptr), _p(b.ptr), st), "gn_coef_parts " + tag)
        L.check(lib.sgd_stats_reduce(_p(p0), n, parts0, c0, _p(s2.ptr), c, 0, st), "stats_reduce 0 " + tag)
        if parts1:
            L.check(lib.sgd_stats_reduce(_p(p1), n, parts1, c1, _p(s2.ptr), c, c0, st), "stats_reduce 1 " + tag)
        L.check(lib.sgd_gn_coef(_p(s2.ptr), _p(gamma), _p(beta), _p(film), cs["film_ld"], n, c, groups, hw, EPS, _p(a2.ptr),
                                _p(b2.ptr), st), "gn_coef " + tag)
        torch.cuda.synchronize()
        bad, errs = [], {}
        folded = slice(0, c if parts1 else c0)       # the channels whose sums the launches fold themselves
        for nm, table in (("fold", sums), ("stats_reduce", s2)):
            got = table.owned().view(n, c, 2)
            errs[nm] = max(max_rel(got[:, folded, k], ref["sums"][:, folded, k]) for k in (0, 1))
            _over(bad, worst, nm, errs[nm], TOL["fold"])
        if c1 > 0 and not parts1 and not torch.equal(sums.tensor().view(torch.int32)[:, 2 * c0:], before):
            bad.append("the sums sgd_chan_stats had written for the source without partials changed")
        for nm, buf, want in (("a", a, ref["a"]), ("b", b, ref["b"]), ("a two launches", a2, ref["a"]), ("b two launches", b2, ref["b"])):
            errs[nm] = max_rel(buf.owned(), want)
            _over(bad, worst, nm.split()[0], errs[nm], TOL["affine"])
        for nm, one, two in (("sums", sums, s2), ("a", a, a2), ("b", b, b2)):
            _over(bad, worst, "one launch vs two", max_rel(one.owned(), two.owned()), TOL["fold"])
        _guards(bad, sums=sums, sums_two_launches=s2, a=a, b=b, a2=a2, b2=b2)
        if report is not None:
            report.append(f"parts case {ci:2d} n {n} c0 {c0:4d} parts0 {parts0:3d} c1 {c1:3d} parts1 {parts1:2d} "
                          + " ".join(f"{k} {v:.2e}" for k, v in errs.items() if "two" not in k))
        if bad:
            failures.append((ci, cs, bad))
    return worst, failures


# ---------------------------------------------------------------------------------------------------------------------
# C, D, F, G. GroupNorm chains
# ---------------------------------------------------------------------------------------------------------------------
def _forward_chain(lib, L, cs, t, tag):
    """sgd_chan_stats per source -> sgd_gn_coef: (per-source device tensors, sums, a, b, film on the device)"""
    n, hw, ct = cs["n"], cs["h"] * cs["w"], sum(cs["srcs"])
    x3 = t["x"].reshape(n, hw, ct)
    xs, off = [], 0
    sums = R.Guarded(n, 2 * ct)
    for c in cs["srcs"]:
        xs.append(x3[..., off:off + c].contiguous().cuda())
        L.check(lib.sgd_chan_stats(_p(xs[-1]), n, hw, c, _p(sums.ptr), ct, off, _stream()), "chan_stats " + tag)
        off += c
    film = R.padded(t["film"][:, :2 * ct], cs["film_ld"]).cuda() if cs["film"] else None
    gamma, beta = t["gamma"].cuda(), t["beta"].cuda()
    a, b = R.Guarded(n, ct), R.Guarded(n, ct)
    L.check(lib.sgd_gn_coef(_p(sums.ptr), _p(gamma), _p(beta), _p(film), cs["film_ld"], n, ct, cs["groups"], hw, EPS, _p(a.ptr),
                            _p(b.ptr), _stream()), "gn_coef " + tag)
    torch.cuda.synchronize()
    return xs, sums, a, b, film, gamma, beta


def _check_forward(cs, t, ref, a, b, bad, worst, tol):
    n, hw, ct = cs["n"], cs["h"] * cs["w"], sum(cs["srcs"])
    y = t["x"].reshape(n, hw, ct).double() * a.owned().double()[:, None] + b.owned().double()[:, None]     # the host forms a x + b
    err = max_rel(y, ref["y"])
    if tol is not None:
        _over(bad, worst, "a x + b", err, tol)
    if cs.get("degenerate"):
        value, grp = cs["degenerate"]
        cpg = ct // cs["groups"]
        ch = slice(grp * cpg, (grp + 1) * cpg)
        want = t["gamma"].double()[None, ch] / torch.sqrt(torch.tensor(EPS, dtype=torch.float32).double())
        if cs["film"]:
            want = want * (1.0 + t["film"].double()[:, ch])
        ga = a.owned().double()[:, ch]
        if not (torch.isfinite(ga).all() and bool(((ga - want).abs() <= ULP * want.abs()).all())):
            bad.append("a of the constant group is not gamma (1 + scale) / sqrt(eps) to fp32 rounding")
        if value == 0.0 and not cs["film"] and not torch.equal(b.owned()[:, ch], t["beta"][None, ch].expand(n, -1)):
            bad.append("b of the all-zero group is not beta bit for bit")
    return err


def run_gn_sweep(name, report=None):
    """a GroupNorm sweep ("forward", "backward", "degenerate") -> ({quantity: worst max_rel}, failures)"""
    L, lib = _lib()
    st = _stream()
    worst, failures = {}, []
    for ci, (cs, t, ref, _) in enumerate(R.sweep_reference(name)):
        n, h, w, ct, groups = cs["n"], cs["h"], cs["w"], sum(cs["srcs"]), cs["groups"]
        hw, tag = h * w, f"{name} case {ci}: {cs}"
        xs, sums, a, b, film, gamma, beta = _forward_chain(lib, L, cs, t, tag)
        bad, errs = [], {}
        errs["y"] = _check_forward(cs, t, ref, a, b, bad, worst, TOL["affine"])
        _guards(bad, sums=sums, a=a, b=b)
        if "gu_mode" in cs:
            silu, gu_mode, drop, seed, acc = cs["silu"], cs["gu_mode"], cs["drop_p"], cs["drop_seed"], cs["accumulate"]
            gu = R.padded(t["gu"], cs["gu_ld"]).cuda()
            gres = R.padded(t["gres"], cs["gres_ld"]).cuda() if t["gres"] is not None else None
            gres_mode = cs["gres_mode"] if gres is not None else 0
            S = R.Guarded(n, 2 * ct)
            off = 0
            for x, c in zip(xs, cs["srcs"]):
                L.check(lib.sgd_gn_bwd_reduce(_p(x), n, h, w, c, ct, off, _p(a.ptr), _p(b.ptr), silu, _p(gu), cs["gu_ld"], gu_mode,
                                              drop, seed, _p(S.ptr), st), "gn_bwd_reduce " + tag)
                off += c
            A, B, Cc, dg, db, A2, B2, C2 = (R.Guarded(n, ct) for _ in range(8))
            dfilm, dfilm2 = ((R.Guarded(n, cs["film_ld"], 2 * ct), R.Guarded(n, cs["film_ld"], 2 * ct)) if cs["film"] else (None, None))
            coef = (_p(sums.ptr), _p(gamma), _p(beta), _p(film), cs["film_ld"], n, ct, groups, hw, EPS)
            L.check(lib.sgd_gn_bwd_coef(_p(S.ptr), 1, *coef, _p(A.ptr), _p(B.ptr), _p(Cc.ptr), _p(dg.ptr), _p(db.ptr),
                                        _p(dfilm.ptr) if dfilm else None, st), "gn_bwd_coef " + tag)
            # the one-launch route: coefficients + scaled column sums, bit for bit the two launches (include/sgdm_hip.h)
            scale = 0.5
            o1, o2, f1, f2 = (R.Guarded(1, ct) for _ in range(4))
            L.check(lib.sgd_colsum_pair(_p(dg.ptr), _p(db.ptr), n, ct, ct, _p(o1.ptr), _p(o2.ptr), 0, scale, st), "colsum_pair " + tag)
            fits = n <= 256 and 8 * n * (ct // groups) + 32 * n + 4 + 2048 <= 64 * 1024
            rc = lib.sgd_gn_bwd_coef_fold(_p(S.ptr), 1, *coef, _p(A2.ptr), _p(B2.ptr), _p(C2.ptr), _p(dfilm2.ptr) if dfilm2 else None,
                                          _p(f1.ptr), _p(f2.ptr), 0, scale, st)
            if (rc == 0) != fits:
                bad.append(("sgd_gn_bwd_coef_fold returned", rc, "fits its LDS bound", fits))
            dsts, off = [], 0
            for x, c in zip(xs, cs["srcs"]):
                dst = R.Guarded(n * hw, cs["dst_off"] + c + cs["dst_pad"], c, cs["dst_off"])
                if acc:
                    dst.fill(t["base"][..., off:off + c])
                L.check(lib.sgd_gn_bwd_apply(_p(x), n, h, w, c, ct, off, _p(a.ptr), _p(b.ptr), silu, _p(gu), cs["gu_ld"], gu_mode, drop,
                                             seed, _p(A.ptr), _p(B.ptr), _p(Cc.ptr), _p(gres), cs["gres_ld"], gres_mode, _p(dst.ptr),
                                             dst.ld, cs["dst_off"], acc, st), "gn_bwd_apply " + tag)
                dsts.append(dst)
                off += c
            torch.cuda.synchronize()
            if rc == 0:
                same = all(torch.equal(u.bits, v.bits) for u, v in ((A, A2), (B, B2), (Cc, C2), (o1, f1), (o2, f2)))
                if dfilm is not None:
                    same = same and torch.equal(dfilm.bits, dfilm2.bits)
                if not same:
                    bad.append("sgd_gn_bwd_coef_fold is not bit for bit sgd_gn_bwd_coef + sgd_colsum_pair")
            got = torch.cat([d.owned().view(n, h, w, c) for d, c in zip(dsts, cs["srcs"])], -1)
            if acc:
                got = got - t["base"]
            errs["dx"] = max_rel(got, ref["dx"])
            errs["dgamma"] = max_rel(dg.owned().double().sum(0), ref["dgamma"])
            errs["dbeta"] = max_rel(db.owned().double().sum(0), ref["dbeta"])
            errs["dgamma fold"] = max_rel(o1.owned().double()[0] / scale, ref["dgamma"])
            errs["dbeta fold"] = max_rel(o2.owned().double()[0] / scale, ref["dbeta"])
            if dfilm is not None:
                errs["dfilm"] = max_rel(dfilm.owned(), ref["dfilm"])
            for nm, err in errs.items():
                if nm != "y":
                    _over(bad, worst, nm.split()[0], err, TOL["gn_bwd"])
            _guards(bad, S=S, A=A, B=B, C=Cc, dgamma_nc=dg, dbeta_nc=db, dfilm=dfilm, dgamma=o1, dbeta=o2,
                    **{f"dst{i}": d for i, d in enumerate(dsts)})
            if cs["rows"]:               # the row-stream reduce on the same tensors: its folded table against the round-1 reduce
                c = cs["srcs"][0]
                chunks = int(lib.sgd_gn_bwd_rows_chunks(n, h, w, c))
                if chunks <= 0:
                    bad.append("sgd_gn_bwd_rows_chunks does not serve the shape")
                else:
                    P = R.Guarded(n * chunks, 2 * ct)
                    L.check(lib.sgd_gn_bwd_reduce_rows(_p(xs[0]), n, h, w, c, ct, 0, _p(a.ptr), _p(b.ptr), silu, _p(gu), cs["gu_ld"],
                                                       drop, seed, chunks, _p(P.ptr), st), "gn_bwd_reduce_rows " + tag)
                    torch.cuda.synchronize()
                    S1 = P.owned().view(n, chunks, ct, 2).double().sum(1)
                    errs["rows"] = max_rel(S1, S.owned().view(n, ct, 2))
                    _over(bad, worst, "reduce_rows vs reduce", errs["rows"], 2e-6)
                    _guards(bad, P=P)
        if report is not None:
            report.append(f"{name} case {ci:2d} n {n} {h:4d}x{w:<2d} srcs {'+'.join(map(str, cs['srcs'])):7s} groups {groups:2d} "
                          + " ".join(f"{k} {v:.2e}" for k, v in errs.items() if "fold" not in k))
        if bad:
            failures.append((ci, cs, bad))
    return worst, failures


def run_offset_sweep(report=None):
    """GroupNorm forward on x = mu + randn: [(case, our error of a x + b, torch fp32's error, a-priori bound at the data's own
    r)], failures.  r <= 4: the standing 5e-6.  r >= 16: within OFFSET_MARGIN x the a-priori bound."""
    L, lib = _lib()
    rows, failures = [], []
    for ci, (cs, t, ref, cond) in enumerate(R.sweep_reference("offset")):
        xs, sums, a, b, *_ = _forward_chain(lib, L, cs, t, f"offset case {ci}: {cs}")
        bad, worst = [], {}
        err = _check_forward(cs, t, ref, a, b, bad, worst, TOL["affine"] if cs["r"] <= 4 else None)
        bound = R.offset_bound(ref["r"])
        if cs["r"] > 4 and not err <= OFFSET_MARGIN * bound:
            bad.append(("a x + b", err, "a-priori bound", bound, "margin", OFFSET_MARGIN))
        _guards(bad, sums=sums, a=a, b=b)
        rows.append((cs, err, cond["y"][0], bound, ref["r"]))
        if report is not None:
            report.append(f"offset r {cs['r']:3d} hw {cs['h']:4d}  largest group r {ref['r']:7.2f}  a x + b {err:.2e}  "
                          f"torch fp32 group_norm {cond['y'][0]:.2e}  a-priori bound {bound:.2e}  error / bound {err / bound:.2f}")
        if bad:
            failures.append((ci, cs, bad))
    return rows, failures


# ---------------------------------------------------------------------------------------------------------------------
# E, F. LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
def run_layernorm_sweep(name, report=None):
    L, lib = _lib()
    st = _stream()
    worst, failures = {}, []
    for ci, (cs, t, ref, _) in enumerate(R.sweep_reference(name)):
        rows, c, acc, tag = cs["rows"], cs["c"], cs["accumulate"], f"{name} case {ci}: {cs}"
        dev = {k: (v.cuda() if v is not None else None) for k, v in t.items()}
        stats, out, dst = R.Guarded(rows, 2), R.Guarded(rows, c), R.Guarded(rows, c)
        gxhat = R.Guarded(rows, c) if cs["gxhat"] else None
        if acc:
            dst.fill(t["base"])
        L.check(lib.sgd_ln_stats(_p(dev["x"]), rows, c, EPS, _p(stats.ptr), st), "ln_stats " + tag)
        L.check(lib.sgd_ln_apply(_p(dev["x"]), _p(dev["gamma"]), _p(dev["beta"]), _p(dev["res"]), rows, c, EPS, _p(out.ptr), st),
                "ln_apply " + tag)
        L.check(lib.sgd_ln_bwd(_p(dev["x"]), _p(dev["g"]), _p(dev["gamma"]), rows, c, EPS, _p(dst.ptr), acc,
                               _p(gxhat.ptr) if gxhat else None, _p(dev["gres"]), st), "ln_bwd " + tag)
        torch.cuda.synchronize()
        bad, errs = [], {}
        errs["out"] = max_rel(out.owned(), ref["out"])
        errs["mean"] = max_rel(stats.owned()[:, 0], ref["mean"])
        errs["rstd"] = max_rel(stats.owned()[:, 1], ref["rstd"])
        for nm in ("out", "mean", "rstd"):
            _over(bad, worst, nm, errs[nm], TOL["ln_fwd"])
        base = t["base"].double() if acc else 0.0
        errs["dx"] = max_rel(dst.owned().double() - base, ref["dst"] - base)
        _over(bad, worst, "dx", errs["dx"], TOL["ln_bwd"])
        if gxhat is not None:
            errs["gxhat"] = max_rel(gxhat.owned(), ref["gxhat"])
            errs["dgamma"] = max_rel(gxhat.owned().double().sum(0), ref["gxhat"].sum(0))
            _over(bad, worst, "gxhat", errs["gxhat"], TOL["ln_bwd"])
            _over(bad, worst, "dgamma", errs["dgamma"], TOL["ln_bwd"])
        _guards(bad, stats=stats, out=out, dst=dst, gxhat=gxhat)
        if cs.get("constant_row"):
            r = cs["constant_row"][0]
            want = 1.0 / float(torch.sqrt(torch.tensor(EPS, dtype=torch.float32).double()))
            if not abs(float(stats.owned()[r, 1]) - want) <= ULP * want:
                bad.append(("rstd of the constant row is not 1 / sqrt(eps) to fp32 rounding", float(stats.owned()[r, 1])))
            if not torch.equal(out.owned()[r], t["beta"] + t["res"][r]):
                bad.append("the output of the constant row is not beta + res bit for bit")
        if report is not None:
            report.append(f"{name} case {ci:2d} rows {rows:2d} c {c:4d} " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        if bad:
            failures.append((ci, cs, bad))
    return worst, failures


# ---------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------
def test_chan_stats_random_geometry():
    _raise(run_chan_stats_sweep()[1])


def test_partial_statistics_random_geometry():
    _raise(run_parts_sweep()[1])


def test_groupnorm_forward_random_geometry():
    _raise(run_gn_sweep("forward")[1])


def test_groupnorm_backward_random_geometry():
    _raise(run_gn_sweep("backward")[1])


def test_layernorm_random_geometry():
    _raise(run_layernorm_sweep("layernorm")[1])


def test_degenerate_groups_and_rows():
    """a group that is exactly zero (a zero_module conv at initialisation) or constant at 0.25, a LayerNorm row that is constant"""
    _raise(run_gn_sweep("degenerate")[1] + run_layernorm_sweep("ln_degenerate")[1])


def test_groupnorm_mean_offset():
    _raise(run_offset_sweep()[1])


def test_refusals():
    """contract checks (include/sgdm_hip.h): each call must return SGD_ERR_ARG and launch nothing -- the host checks return
    before any launch, and the refused GroupNorm-backward geometries are exactly the ones a launch would read out of bounds
    with.  Every pointer lies inside one large zeroed buffer all the same."""
    L, lib = _lib()
    st = _stream()
    arena = torch.zeros(16 * 16384, device="cuda")
    at = lambda i: C.c_void_p(arena.data_ptr() + 4 * 16384 * i)
    # sgd_gn_coef_parts: more than 8192 channels; a channel count whose 24 bytes of LDS per channel exceed 160 KB
    for c0, c1 in ((8192, 32), (7168, 0), (6848, 0)):
        assert lib.sgd_gn_coef_parts(at(0), 2, c0, at(1), 2, c1, at(2), at(3), at(4), None, 0, 1, 32, 16, EPS, at(5), at(6), st) == 1, (c0, c1)
    # LayerNorm: a row longer than the 16 registers x 64 lanes that hold it
    assert lib.sgd_ln_stats(at(0), 2, 1025, EPS, at(1), st) == 1
    assert lib.sgd_ln_apply(at(0), at(1), at(2), at(3), 2, 1025, EPS, at(4), st) == 1
    assert lib.sgd_ln_bwd(at(0), at(1), at(2), 2, 1025, EPS, at(3), 0, at(4), at(5), st) == 1
    # GroupNorm backward: n 1, c 4; x / gu / gres / dst in slots of their own

    def reduce(h, w, gu_mode):
        return lib.sgd_gn_bwd_reduce(at(0), 1, h, w, 4, 4, 0, at(1), at(2), 1, at(3), 4, gu_mode, 0.0, 0, at(4), st)

    def apply(h, w, gu_mode, gres, gres_mode):
        return lib.sgd_gn_bwd_apply(at(0), 1, h, w, 4, 4, 0, at(1), at(2), 1, at(3), 4, gu_mode, 0.0, 0, at(5), at(6), at(7),
                                    at(8) if gres else None, 4, gres_mode, at(9), 4, 0, 0, st)

    for h, w in ((3, 4), (4, 3), (1, 1), (5, 5)):            # the pooled mode with an odd h or w
        assert reduce(h, w, R.RS_AVGPOOL2) == 1, ("reduce", h, w)
        assert apply(h, w, R.RS_AVGPOOL2, False, 0) == 1, ("apply, gu_mode", h, w)
        assert apply(h, w, R.RS_NONE, True, R.RS_AVGPOOL2) == 1, ("apply, gres_mode", h, w)
        assert apply(h, w, R.RS_UP2, True, R.RS_AVGPOOL2) == 1, ("apply, gres_mode", h, w)
    for mode in (-1, 3, 4, 5, 1 << 20):                      # not one of SGD_RS_NONE / AVGPOOL2 / UP2
        assert reduce(4, 4, mode) == 1, ("reduce", mode)
        assert apply(4, 4, mode, False, 0) == 1, ("apply, gu_mode", mode)
        assert apply(4, 4, R.RS_NONE, True, mode) == 1, ("apply, gres_mode", mode)
    torch.cuda.synchronize()
    assert float(arena.abs().max()) == 0.0, "a refused call launched"
