"""CPU: the conditions that keep tests/test_hip_ingest_paths.py from passing vacuously.

That file holds every count-ingest path to the dense answer by equality of engines.  Equality says nothing where the two paths cannot
differ: a batch permutation that is its own inverse hides a swap of the scatter kernel's table (pos: cell -> position) with the pack
kernel's (ord: position -> cell); a CSR matrix that scipy canonicalised on the way never shows the kernel an explicit zero or a
64-entry row; a "strided" tensor that became contiguous takes the one upload branch every other test takes.  Here, on the host:
  * helpers.sparse_edge_counts plants every feature its docstring names, in the form the engine is handed;
  * on every interleaved case the two tables differ, and a scatter with the wrong one misplaces at least a quarter of the cells;
  * the shards of group b lack whole batches (planted) or hold every batch in permuted order (interleaved);
  * group h's entry counts lie on the intended sides of OVF_CAP;
  * group f's four forms have the strides the GPU test asserts and take different branches of vc_set_counts."""
import os
import re

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import test_hip_ingest_paths as P
from tests.test_hip_batch_paths import _case
from velocycle_amd.engine import shard_bounds


# ---- sparse_edge_counts ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [31, 32])
def test_sparse_edge_counts_plants_every_feature(seed):
    Nc, Ng = P.SPARSE_NC, P.SPARSE_NG
    dense, raw = H.sparse_edge_counts(Nc, Ng, seed)
    assert dense.shape == (Nc, Ng) and dense.dtype == np.float32 and raw.shape == (Nc, Ng) and raw.data.dtype == np.float32
    c0, c1 = shard_bounds(Nc, 1, 3)
    # what the engine hands to the kernel: this rank's rows with duplicates summed, explicit zeros kept (engine._setup)
    seen = raw.copy()
    seen.sum_duplicates()
    n_raw, n_seen = np.diff(raw.indptr), np.diff(seen.indptr)
    for c in (0, Nc - 1, c0, c1 - 1):                                   # empty cells at both ends of the matrix and of shard 1
        assert n_raw[c] == 0 and n_seen[c] == 0
    for lo, hi in ((0, c0), (c0, c1)):                                  # the planted lengths, on rank 0 and on rank 1 of 3
        assert set(H.SPARSE_EDGE_ROW_LENGTHS) <= set(n_seen[lo:hi].tolist()), sorted(set(n_seen[lo:hi].tolist()))
    assert {0, 1, 63, 64, 65} <= set(n_seen.tolist()) and n_seen.max() >= 129
    # one gene without any entry; the last gene (the ragged block at four genes per lane: 300 = 256 + 44) with entries on both ranks
    per_gene = np.bincount(raw.indices, minlength=Ng)
    assert per_gene[H.SPARSE_EDGE_EMPTY_GENE] == 0 and (np.delete(per_gene, H.SPARSE_EDGE_EMPTY_GENE) > 0).all()
    assert (dense[:c0, Ng - 1] > 0).any() and (dense[c0:c1, Ng - 1] > 0).any() and Ng - 1 >= 256
    # explicit zeros and duplicates are in the raw CSR ...
    assert int((raw.data == 0).sum()) >= 20
    assert raw.nnz - seen.nnz >= 20 and not raw.has_canonical_format
    assert int((seen.data == 0).sum()) >= 20                            # ... the zeros still in what the kernel sees ...
    canon = seen.copy()
    canon.eliminate_zeros()                                             # ... and gone from the canonical form of preprocessing._csr_counts
    assert int((canon.data == 0).sum()) == 0 and canon.nnz == int((dense != 0).sum()) and canon.has_canonical_format
    # rows stored in descending order (each of the planted lengths on shard 1), and rows in no order at all
    desc = [c for c in range(Nc) if n_raw[c] >= 2 and (np.diff(raw.indices[raw.indptr[c]:raw.indptr[c + 1]]) < 0).all()]
    assert {int(n_raw[c]) for c in desc} >= set(H.SPARSE_EDGE_ROW_LENGTHS) - {1} and all(c0 <= c < c1 for c in desc if n_raw[c] >= 63)
    # the dense matrix is what the CSR stands for: the float64 sum of the entries, cast to float32; duplicates ADD
    assert np.array_equal(dense, raw.toarray()) and np.array_equal(dense, canon.toarray())
    want = np.zeros((Nc, Ng))
    np.add.at(want, (np.repeat(np.arange(Nc), n_raw), raw.indices), raw.data.astype(np.float64))
    assert np.array_equal(dense, want.astype(np.float32))
    rows = np.repeat(np.arange(Nc), n_raw)
    key = rows.astype(np.int64) * Ng + raw.indices
    uniq, cnt = np.unique(key, return_counts=True)
    twice = uniq[cnt == 2]
    assert twice.size >= 20 and (cnt <= 2).all()
    for k in twice[:5]:
        parts = raw.data[key == k]
        assert parts.size == 2 and (parts > 0).all() and dense[k // Ng, k % Ng] == parts.sum() > parts.max()
    # counts stay small integers: uint16 storage and the dense histogram tables remain selectable
    assert dense.max() <= 24 and np.array_equal(dense, np.floor(dense))


def test_sparse_edge_specs_hand_the_raw_csr_to_the_engine():
    for kind in ("phase", "vjoint"):
        dense, csr = P.sparse_edge_specs(kind)
        assert csr.S is None and csr.U is None and not csr.S_csr.has_canonical_format
        assert torch.equal(dense.S, torch.tensor(csr.S_csr.toarray()).t()) and dense.S.shape == (P.SPARSE_NG, P.SPARSE_NC)
        assert (dense.U is None) == (kind == "phase") == (csr.U_csr is None)
        if dense.U is not None:
            assert torch.equal(dense.U, torch.tensor(csr.U_csr.toarray()).t()) and not torch.equal(dense.U, dense.S)
        # slicing a rank's rows (engine._setup) copies: the caller's matrix is not canonicalised behind its back
        part = csr.S_csr.tocsr()[0:P.SPARSE_NC]
        part.sum_duplicates()
        assert part.nnz < csr.S_csr.nnz and not csr.S_csr.has_canonical_format


# ---- groups a, b: the batch permutations ---------------------------------------------------------------------------------------------

def _interleaved_specs():
    out = [(f"{m} Nb={Nb} Ng={Ng}", _case(m, layout, Nb, Ng)[0]) for m, layout, Nb, Ng in P.batch_cases() if layout == "interleaved"]
    assert len(out) == 2 * len(P.BATCH_MODELS)
    return out


def test_interleaved_cases_have_a_permutation_that_is_not_its_own_inverse():
    for label, spec in _interleaved_specs():
        ids = P.batch_ids(spec)
        Nc = ids.size
        order, pos = P.batch_order(ids)
        assert np.array_equal(np.sort(ids), ids[order]) and np.array_equal(order[pos], np.arange(Nc))       # ord sorts, pos inverts it
        assert not np.array_equal(order, pos), label
        # the scatter kernel's write, dst[:, table[c]] = src[:, c], with the right table and with the pack kernel's
        M = spec.S.numpy()
        right, wrong = np.empty_like(M), np.empty_like(M)
        right[:, pos] = M
        wrong[:, order] = M
        assert np.array_equal(right, M[:, order])                        # = what vc_pack_counts_kernel stores: position p holds cell ord[p]
        differ = int((right != wrong).any(axis=0).sum())
        assert differ >= Nc / 4, (label, differ, Nc)
        print(f"[ingest cases] {label}: a scatter through ord misplaces {differ} of {Nc} cells")


def test_contiguous_and_planted_cases_need_no_permutation():
    for m, layout, Nb, Ng in P.batch_cases():
        if layout != "interleaved":
            ids = P.batch_ids(_case(m, layout, Nb, Ng)[0])
            assert (np.diff(ids) >= 0).all(), (m, layout)                 # pos == nullptr: the identity


def test_shards_lack_batches_or_reorder():
    for layout, Nb in P.SHARD_LAYOUTS:
        for m in P.BATCH_MODELS:
            spec = _case(m, layout, Nb, P.batch_ng(layout, Nb))[0]
            ids = P.batch_ids(spec)
            present = set(np.unique(ids).tolist())
            for rank in (1, 2):
                c0, c1 = shard_bounds(ids.size, rank, 3)
                mine = ids[c0:c1]
                if layout == "planted":
                    # a rank lacks whole batches, and its own cells are in batch order already
                    assert len(present - set(mine.tolist())) >= 1 and (np.diff(mine) >= 0).all(), (m, rank)
                else:
                    assert set(mine.tolist()) == present, (m, rank)
                    order, pos = P.batch_order(mine)
                    assert not np.array_equal(order, pos) and (pos != np.arange(mine.size)).sum() >= mine.size / 4, (m, rank)
            if layout == "planted":
                assert len(present) == Nb - 1                              # (batch 2 of the planted layout has no cell at all)


def test_lognormal_batch_cases_are_interleaved():
    from tests.test_hip_sweep import _problem
    for kind, seed in (("phase", 9103), ("velocity", 9113)):
        p = _problem(kind, "meanfield", "Lognormal", 1, 1 if kind == "velocity" else 0, 3, 2 if kind == "velocity" else 0, [],
                     Nc=661, Ng=70, seed=seed)
        order, pos = P.batch_order(p.Db.argmax(0).numpy())
        assert not np.array_equal(order, pos)


# ---- group h: the overflow cap --------------------------------------------------------------------------------------------------------

def test_cap_cases_lie_on_both_sides_of_the_overflow_cap():
    src = open(os.path.join(os.path.dirname(H.GOLDEN), "..", "velocycle_amd", "csrc", "vc_engine.hip")).read()
    m = re.search(r"static const unsigned OVF_CAP = 1u << (\d+);", src)
    assert m and (1 << int(m.group(1))) == P.OVF_CAP == 4194304
    assert "novf[0] > OVF_CAP || novf[1] > OVF_CAP" in src               # the trigger: strictly more entries than the list holds
    assert P.CAP_NC_OVER * P.CAP_NG == 4200000 > P.OVF_CAP > P.CAP_NC_UNDER * P.CAP_NG == 4180000
    spec = P.cap_spec(P.CAP_NC_UNDER)
    S = spec.S.numpy()
    assert S.shape == (P.CAP_NG, P.CAP_NC_UNDER) and S.dtype == np.float32
    assert (S != np.floor(S)).all() and (S > 0).all() and np.isfinite(S).all()          # every entry is an overflow entry
    assert spec.kind == "phase" and spec.noisemodel == "NegativeBinomial"


# ---- group f: strides -------------------------------------------------------------------------------------------------------------------

def test_stride_forms_take_different_upload_branches():
    Ng, Nc = P.STRIDE_NG, P.STRIDE_NC
    base = P.stride_base_spec()
    assert base.S.shape == (Ng, Nc) and base.U.shape == (Ng, Nc) and base.kind == "velocity"
    branches = {}
    for form in P.STRIDE_FORMS:
        spec = P.stride_spec(form, "cpu")
        assert spec.S.stride() == spec.U.stride() == P.stride_of(form), (form, spec.S.stride())
        assert torch.equal(spec.S, base.S) and torch.equal(spec.U, base.U)
        gs, cs = spec.S.stride()
        assert gs > 0 and cs > 0                                           # engine._setup keeps such views as they are
        branches[form] = P.upload_branch(gs, cs, Ng, Nc)
        # a shard's view (engine._setup: S[:, c0:c1]) keeps the strides: the same branch on the shard's own Nc, where a row of the
        # contiguous matrix is padded too (only this rank's columns of every row are uploaded)
        c0, c1 = shard_bounds(Nc, 1, 3)
        assert spec.S[:, c0:c1].stride() == (gs, cs)
        assert P.upload_branch(gs, cs, Ng, c1 - c0) == branches[form].replace("_tight", "_padded")
    assert branches == {"gene_major": "rows_of_cells_tight", "cell_major_T": "rows_of_genes", "column_slice": "rows_of_cells_padded",
                        "both_strided": "whole_span"}
    # the conditions of vc_set_counts, on (gs, cs, Ng, Nc)
    gs, cs = P.stride_of("cell_major_T")
    assert gs == 1 and cs >= Ng
    for form in ("gene_major", "column_slice"):
        gs, cs = P.stride_of(form)
        assert not (gs == 1 and cs >= Ng) and cs == 1 and gs >= Nc
    assert P.stride_of("gene_major")[0] == Nc < P.stride_of("column_slice")[0]
    gs, cs = P.stride_of("both_strided")
    assert gs > 1 and cs > 1 and not (gs == 1 and cs >= Ng) and not (cs == 1 and gs >= Nc)
