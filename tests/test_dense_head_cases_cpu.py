"""The dense head's case table (``dense_head_ref.py``) checked without a GPU: every class of width has its widths and its cases,
the two branch conditions give each case the class it claims, a float32 product of every case's operands meets both gates, and the
gates refuse the two wrong kernels the sweep exists for -- the staging race of H = 8m - 1 lost (``pooled[r+1][0]`` a pad value) and a
k-slice dropped.  The gates of the other tail launches are checked on float32 sums the same way."""
import pytest
import torch

import dense_head_ref as dr

CASES = [pytest.param(name, c, id="%s-%s" % (name, dr.case_id(c))) for name, c in dr.CASES]
# class -> (16-byte staging on a 16-byte aligned layout with ldp % 4 == 0, 16-byte product)
EXPECT = {"8m-1": (False, False), "mult8-prod16": (True, True), "mult8-prod1": (True, False), "scalar-prod16": (False, True),
          "narrow": (False, False), "ordinary": (False, False)}


def test_every_class_has_its_widths_batches_layouts_and_sums():
    assert set(dr.TABLE) == set(dr.REQUIRED) == set(EXPECT)
    ids = [dr.case_id(c) for _, c in dr.CASES]
    assert len(set(ids)) == len(ids)
    for name, widths in dr.REQUIRED.items():
        cases = dr.TABLE[name]
        assert cases, name
        own = [c for c in cases if name != "8m-1" or dr.defect_class(c)]       # 8m - 1: the layout the parent staged by 16 bytes
        for H in widths:
            assert {c.B for c in own if c.H == H} >= set(dr.BATCHES), (name, H)
        assert {c.H for c in own if c.B >= dr.MANY} >= {widths[0], widths[-1]}, name
        assert {c.C for c in own} >= set(dr.CLASSES_C), name
        assert {c.bias for c in own} == {True, False}, name
        assert {c.pad_p for c in cases if not c.offset} >= {0, 1, 3, 4}, name
        assert any(c.offset and dr.pointer_offset(c) == 4 for c in cases), name
        assert any(c.pad_w == 3 for c in cases) and any(c.pad_l == 3 for c in cases), name
    # the defect class by its own description: pad_p = 1, aligned, 16-byte staged by the parent's condition and by it alone
    defect = [c for c in dr.TABLE["8m-1"] if dr.defect_class(c)]
    assert {c.H for c in defect if c.pad_p == 1 and not c.offset} == {7, 15, 39, 767, 1023}
    assert all(not dr.staging16(c) for c in defect)
    # element staging with the 16-byte product, k-slices that are empty
    assert {c.H for c in dr.TABLE["scalar-prod16"]} == {52, 116, 180}
    assert [dr.empty_slices(H) for H in (52, 116, 180, 1, 2, 5, 768, 1024)] == [3, 1, 1, 15, 14, 11, 0, 0]
    # the LDS bound: H = 1024 is exactly 64 KiB
    assert (dr.ROWS * 1024 + dr.WAVES * dr.ROWS * 64) * 4 == 64 * 1024 and 1024 in dr.REQUIRED["mult8-prod16"]
    # the final sum: one workgroup's stride of 1024 threads met exactly, passed by one, and passed several times
    sums = [c for _, c in dr.CASES if c.n_part_spec]
    assert sorted(dr.n_part(c) for c in sums) == sorted(dr.N_PARTS) == [1, 63, 1024, 1025, 6240]
    assert [(c.B, c.n_part_spec) for c in sums if dr.n_part(c) > 1024] and max(dr.n_part(c) for c in sums) >= 6000


@pytest.mark.parametrize("name,c", CASES)
def test_the_predicates_give_the_class_the_case_claims(name, c):
    assert dr.width_class(c) == name
    aligned = (c.H + c.pad_p) % 4 == 0 and not c.offset
    staging, product = EXPECT[name]
    assert dr.staging16(c) == (staging and aligned)
    assert dr.product16(c) == product
    # the fix changes the staging of H = 8m - 1 on aligned layouts and of nothing else
    assert (dr.staging16_parent(c) != dr.staging16(c)) == (name == "8m-1" and aligned) == dr.defect_class(c)
    # the index walk of the 16-byte staging, as the kernel does it: no float of a row's second half past the row
    if dr.staging16(c):
        hb = (c.H + 1) >> 1
        assert hb % 4 == 0 and max(k + 3 for kb in (0, hb) for k in range(kb, min(kb + hb, c.H), 4)) == c.H - 1
    if dr.defect_class(c):
        hb = (c.H + 1) >> 1
        assert max(k + 3 for k in range(hb, c.H, 4)) == c.H          # the parent's walk: one float into the next row


def test_the_parents_condition_overran_exactly_the_128_widths_8m_minus_1():
    bad = []
    for H in range(1, 1025):
        hb = (H + 1) >> 1
        if hb % 4 == 0 and any(k + 3 >= H for kb in (0, hb) for k in range(kb, min(kb + hb, H), 4)):
            bad.append(H)
    assert bad == list(range(7, 1024, 8)) and len(bad) == 128


@pytest.mark.parametrize("name,c", CASES)
def test_a_float32_product_meets_both_gates_and_the_wrong_kernels_miss_them(name, c):
    p, wt, bias, part = dr.operands(c)
    assert float(p[:, 0].abs().min()) >= 1.0 and float(p[:, 0].abs().max()) <= 2.0
    assert float(wt[0].abs().min()) >= 1.0 / c.H ** 0.5 * (1 - 1e-6)
    plain = p @ wt if bias is None else p @ wt + bias
    r = dr.ratios(c, p, wt, bias, plain)
    print("%s: float32 product at %.3f of the derived gate, %.3f of the project's" % (dr.case_id(c), r["derived"], r["project"]))
    dr.assert_gates(c, r, "float32 product")
    ref, S = dr.statement64(p, wt, bias)
    gate = dr.derived_gate(S, c.H)
    if c.B > 1:
        # the race lost: EVERY element of EVERY row it touches is outside the derived gate (and the project's)
        q = dr.defect_signature(p)
        wrong = q @ wt if bias is None else q @ wt + bias
        hit = torch.arange(c.B) % dr.ROWS != 0
        assert bool(((wrong.double() - ref).abs()[hit] > gate[hit]).all()), dr.case_id(c)
        assert bool(((wrong.double() - ref).abs()[hit] > dr.project_gate(ref)).all()), dr.case_id(c)
        assert torch.equal(wrong[~hit], plain[~hit])
    for w in {0, (c.H - 1) // (-(-c.H // dr.WAVES))}:          # the first and the last slice that holds a column
        q = dr.slice_dropped(p, w)
        short = q @ wt if bias is None else q @ wt + bias
        assert dr.worst_ratio(short, ref, gate) > 1.0, (dr.case_id(c), w)
    if part is not None:
        n = dr.n_part(c)
        assert part.numel() == n
        xy = part.sum() / c.B
        rx = dr.xy_ratio(part, c.B, xy)
        assert rx == rx and rx <= 1.0, rx
        if n > 1:
            # the final sum's own wrong kernel: one pass of the 1024 threads and no stride (n <= 1024: the last partial left out)
            assert dr.xy_ratio(part, c.B, part[:min(n - 1, 1024)].sum() / c.B) > 1.0


@pytest.mark.parametrize("M", dr.COLSUM_M)
def test_colsum_gate_on_a_float32_sum(M):
    x = torch.randn(M, 65, generator=torch.Generator().manual_seed(M))
    r = dr.colsum_ratio(x, x.sum(0))
    assert r == r and r <= 1.0, r
    if M > 1:
        assert dr.colsum_ratio(x, x[:-1].sum(0)) > 1.0


@pytest.mark.parametrize("B", dr.OVERLAP_B)
@pytest.mark.parametrize("F", dr.OVERLAP_F)
def test_overlap_gate_on_a_float32_sum(B, F):
    gen = torch.Generator().manual_seed(B + F)
    x1, y1 = 0.5 + 0.5 * torch.rand(B, F, generator=gen), 0.5 + 0.5 * torch.rand(B, F, generator=gen)
    r = dr.overlap_ratio(x1, y1, (x1 * y1).sum(1).mean())
    assert r == r and r <= 1.0, r
    if F > 1:
        assert dr.overlap_ratio(x1, y1, (x1[:, :-1] * y1[:, :-1]).sum(1).mean()) > 1.0
