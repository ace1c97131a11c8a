"""The head-bound checker of tests/headbound.py, tested on itself: CPU only, no kernels.  The float64 restatement of the heads reproduces the reference modules' own
outputs (tests/golden/heads.npz, magface.npz) and its jacobian is the derivative of its logit; the oracle's own 16-bit result passes its bounds; the same result with one
planted fault -- a dropped column at each edge, a column holding its neighbour's values, a zeroed scalar tail, one row's hard negative ignored, a target taken from the
neighbouring column, the shard's class count in the smoothing term -- is rejected, entry by entry and, where the fault moves a whole column or pair, in dW and dfeats."""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import headbound as hb

G = Path(__file__).resolve().parent / "golden"
GOLDEN = {"arcface": dict(m=0.35, m_am=0.0, s=32.0), "circle": dict(m=0.25, s=256.0), "mv_am": dict(m=0.35, t=1.12, s=32.0), "mv_arc": dict(m=0.35, t=1.12, s=32.0)}
EPS, B, C, D = 0.1, 24, 5003, 128
_ENT, _E2E = {}, {}


def entries(mode):
    if mode not in _ENT:
        pc = hb.planted_cos(B, C, mode, 1)
        ref = hb.head_rows(pc.h, pc.cos, pc.labels, EPS, 1.0 / B)
        o32 = hb.head_rows(pc.h, pc.cos, pc.labels, EPS, 1.0 / B, dtype=torch.float32)
        orc = o32.dcos.bfloat16()
        _ENT[mode] = (pc, ref, o32, orc, hb.bound16(hb.entry_errors(orc, ref.dcos, ref.s_dcos)))
    return _ENT[mode]


def e2e(mode):
    if mode not in _E2E:
        ph = hb.planted_head(D, C, mode, 2)
        ref = hb.head_e2e(ph.h, ph.feats, ph.weight, ph.labels, EPS)
        orc = hb.head_e2e(ph.h, ph.feats, ph.weight, ph.labels, EPS, dtype=torch.float32, fmt=torch.bfloat16)
        _E2E[mode] = (ph, ref, orc, hb.e2e_bounds(ref, orc))
    return _E2E[mode]


@pytest.mark.parametrize("tag", hb.MODES)
def test_restatement_reproduces_the_reference_modules(tag):
    """logits, loss, dfeats and dweight of the reference's own float32 run.  Bounds: a float32 logit is a handful of roundings of terms of size s, |d logit| <= 8 eps32 s;
    the loss a mean of lse - logit, 8 eps32 |loss| and the same in absolute terms; a gradient row or column in units of its absolute-value scale carries the float32
    rounding of p (|d logit|, relative) and of the two products' sums: 2e-5, three orders below what a wrong branch or jacobian costs (O(1))"""
    z = np.load(G / "heads.npz")
    t = lambda n: torch.from_numpy(z[n])
    h = hb.head(tag, **GOLDEN[tag])
    r = hb.head_e2e(h, t("feats"), t(f"{tag}_weight"), t("labels"))
    assert float((r.r.logit - t(f"{tag}_logits").double()).abs().max()) <= 8 * hb.EPS32 * h.s
    assert abs(float(r.r.loss.mean()) - float(z[f"{tag}_loss"])) <= 8 * hb.EPS32 * (1.0 + abs(float(z[f"{tag}_loss"])))
    assert float(hb.row_errors(t(f"{tag}_dfeats"), r.dfeats, r.s_dfeats).max()) <= 2e-5
    assert float(hb.col_errors(t(f"{tag}_dweight"), r.dweight, r.s_dweight).max()) <= 2e-5


def test_restatement_reproduces_the_reference_magface():
    """magface.py's run: the magnitude-aware margin, its own gradient path and the regulariser's (feature norms from 3.8 to 142: below l_a, inside, above u_a)"""
    z = np.load(G / "magface.npz")
    t = lambda n: torch.from_numpy(z[n])
    h = hb.head("arcface", m_am=0.0)
    r = hb.head_e2e(h, t("feats"), t("weight"), t("labels"), mag=hb.MAG)
    x = t("feats").double().norm(dim=1).clamp(hb.MAG["l_a"], hb.MAG["u_a"])
    reg = hb.MAG["lamda"] * (x / hb.MAG["u_a"] ** 2 + 1.0 / x)
    assert float((r.r.logit - t("logits").double()).abs().max()) <= 8 * hb.EPS32 * h.s
    assert float((reg - t("reg")[:, 0].double()).abs().max()) <= 8 * hb.EPS32 * float(reg.max())
    assert abs(float(r.r.loss.mean() + reg.mean()) - float(z["loss"])) <= 8 * hb.EPS32 * (1.0 + abs(float(z["loss"])))
    assert float(hb.row_errors(t("dfeats"), r.dfeats, r.s_dfeats).max()) <= 2e-5
    assert float(hb.col_errors(t("dweight"), r.dweight, r.s_dweight).max()) <= 2e-5


@pytest.mark.parametrize("mode", ["arcface", "mv_am", "mv_arc"])
def test_jacobian_is_the_derivative_of_the_logit(mode):
    """central differences in float64 on the planted matrix (every branch: clamp, fallback, both sides of the MV threshold); every entry, moved by 1e-7 <= GUARD, stays in
    its branch.  CircleLoss detaches alpha, so its jacobian is not the derivative of its logit; the golden gradients above pin it."""
    pc = entries(mode)[0]
    c = pc.cos.double()
    d = 1e-7
    _, jac, _ = hb.margin_terms(pc.h, c, pc.labels)
    fd = (hb.margin_terms(pc.h, c + d, pc.labels)[0] - hb.margin_terms(pc.h, c - d, pc.labels)[0]) / (2 * d)
    assert float((fd - jac).abs().max()) <= 1e-5 * pc.h.s
    assert float(jac[pc.special["above_1"]]) == (0.0 if mode == "arcface" else pc.h.s * pc.h.t)


@pytest.mark.parametrize("mode", hb.MODES)
def test_planted_cos_plants_what_it_says(mode):
    pc, ref, _, _, _ = entries(mode)
    rows = torch.arange(B)
    assert set(pc.labels.tolist()) == set(pc.edges)                                      # every edge column is a target ...
    assert {j for r, j in pc.pairs if int(pc.labels[r]) != j} == set(pc.edges)             # ... and the hard negative of another row
    n = len(pc.edges)
    p = ref.p[torch.tensor([q[0] for q in pc.pairs[:2 * n]]), torch.tensor([q[1] for q in pc.pairs[:2 * n]])]
    assert 0.1 <= float(p.min()) and float(p.max()) <= 0.9                                # O(1) probability on both, in the n rows without special entries
    if mode in ("arcface", "circle"):
        assert float(ref.jac[pc.special["above_1"]]) == 0.0 and float(ref.jac[pc.special["below_-1"]]) == 0.0
    if mode == "circle":
        assert float(ref.jac[pc.special["below_-m"]]) == 0.0
    if mode == "arcface":
        r, j = pc.special["fallback_target"]
        assert float(ref.logit[r, j]) == pytest.approx(pc.h.s * (float(pc.cos[r, j]) - pc.h.m_am))
    if mode in ("mv_am", "mv_arc"):
        assert float(ref.jac[pc.special["above_thr"]]) == pc.h.s * pc.h.t and float(ref.jac[pc.special["below_thr"]]) == pc.h.s
    assert bool((ref.hot[rows, pc.labels] == 1).all())


@pytest.mark.parametrize("mode", hb.MODES)
def test_the_oracle_itself_passes(mode):
    pc, ref, o32, orc, bnd = entries(mode)
    assert hb.check("dcos", hb.entry_errors(orc, ref.dcos, ref.s_dcos), bnd, what="oracle") == pytest.approx(1.0)
    b32 = hb.bound32(hb.entry_errors(o32.dcos, ref.dcos, ref.s_dcos))
    hb.check("dcos32", hb.entry_errors(o32.dcos, ref.dcos, ref.s_dcos), b32, hb.LSE_FACTOR, "float32 torch")
    ph, r64, o16, b = e2e(mode)
    hb.assert_shares(r64, ph.pairs)
    hb.assert_sensitive(r64, ph.pairs, b, mode)
    for kind, e in hb.e2e_errors(o16.dfeats, o16.dweight, r64).items():
        assert hb.check(kind, e, b[kind], what="oracle") == pytest.approx(1.0)
    df, dw = hb.backward_from_dcos(o16, o16.d16.bfloat16())                              # the path the planted faults take reproduces the oracle
    assert torch.equal(df, o16.dfeats) and torch.equal(dw, o16.dweight)


def _rejected(name, e, bnd):
    with pytest.raises(AssertionError):
        hb.check(name, e, bnd, what="planted")


@pytest.mark.parametrize("mode", hb.MODES)
def test_every_planted_entry_fault_is_rejected(mode):
    pc, ref, o32, orc, bnd = entries(mode)
    err = lambda bad: hb.entry_errors(bad, ref.dcos, ref.s_dcos)
    for j in pc.edges:
        _rejected(f"drop {j}", err(hb.plant("drop_col", orc, C, col=j)), bnd)
        _rejected(f"shift {j}", err(hb.plant("shift_col", orc, C, col=j)), bnd)
    _rejected("tail", err(hb.plant("zero_tail", orc, C)), bnd)
    r, j = pc.pairs[1]                                                                   # row 0's hard negative
    _rejected("negative", err(hb.plant("ignore_pair", orc, C, row=r, col=j)), bnd)
    for r in (0, len(pc.edges) - 1):
        lab = pc.labels.clone()
        lab[r] = lab[r] + 1 if lab[r] + 1 < C else lab[r] - 1
        other = hb.head_rows(pc.h, pc.cos, lab, EPS, 1.0 / B, dtype=torch.float32).dcos[r]
        _rejected("neighbour", err(hb.plant("replace_row", orc, C, row=r, other=other)), bnd)
        other = hb.head_rows(pc.h, pc.cos, pc.labels, EPS, 1.0 / B, C_total=2504, dtype=torch.float32).dcos[r]
        _rejected("shard C", err(hb.plant("replace_row", orc, C, row=r, other=other)), bnd)


@pytest.mark.parametrize("mode", hb.MODES)
def test_every_planted_column_fault_is_rejected(mode):
    ph, ref, orc, bnd = e2e(mode)
    d16 = orc.d16.bfloat16()

    def both(bad, kinds=("dfeats", "dweight")):
        df, dw = hb.backward_from_dcos(orc, bad)
        e = hb.e2e_errors(df, dw, ref)
        for kind in kinds:
            _rejected(kind, e[kind], bnd[kind])

    for j in ph.edges:
        both(hb.plant("drop_col", d16, C, col=j))
        both(hb.plant("shift_col", d16, C, col=j))
    both(hb.plant("drop_col", d16, C, col=2000), kinds=("dweight",))                     # an ordinary column comes back zero
    both(hb.plant("zero_tail", d16, C))
    for r, j in ph.pairs:
        both(hb.plant("ignore_pair", d16, C, row=r, col=j))
    lab = ph.labels.clone()
    lab[3] += 1
    other = hb.head_e2e(ph.h, ph.feats, ph.weight, lab, EPS, dtype=torch.float32, fmt=torch.bfloat16).d16[3]
    both(hb.plant("replace_row", d16, C, row=3, other=other))
