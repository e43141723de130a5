"""Enrichment of gene clusters in annotation terms on the device: the "Pathway Enrichment: analyze GO term enrichment within
UMAP clusters" step the vcf2embed notebook lists as future work, over its gene -> GO term lists.

  membership(annotations, universe)        the term-major CSR of an annotation restricted to a gene universe, and the term names;
  hypergeom(labels, membership)            for every (term, cluster) cell the overlap and the hypergeometric tail of it:
                                           count, term_size, cluster_size, log_p, p;
  enrich(labels, annotations, universe)    the above plus the fold enrichment, the Benjamini-Hochberg q over all tested cells and
                                           a tidy frame of the significant (cluster, term) rows, sorted by q.

Two entries of include/vf_hip_enrich.h do the work: ops.enrich_counts (the overlap of every term with every
cluster, and with the universe; called once more with the one term that lists every gene for the cluster sizes) and
ops.hypergeom_tail (one thread per cell: a sum of + * / in fp64 that runs away from the mode, on top of a table of
log-factorials that this module computes on the host with math.lgamma).  The logarithm of p never underflows; p = exp(log_p)
may.  The q values are fp64 torch on the device -- a sort and a reversed running minimum -- and follow
scipy.stats.false_discovery_control(method="bh") operation for operation.  There is no CPU path: without a GPU the calls raise,
after their arguments have been checked.  scipy is not imported: tests/enrich_cases.py holds the two together.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import ops

MAX_K, MAX_N = ops.ENRICH_MAX_K, ops.ENRICH_MAX_N
ALTERNATIVES = ("greater", "less")


class Membership(NamedTuple):
    """A term-major CSR annotation over a universe of `genes` rows: term t lists the rows gene[termptr[t] : termptr[t + 1]],
    ascending, each once; terms[t] names it."""
    termptr: np.ndarray        # int64 [T + 1]
    gene: np.ndarray           # int32 [nnz]
    terms: list                # T names
    genes: int                 # G, the universe


# ---- argument checks -------------------------------------------------------------------------------------------------------------
def _int_in(value, name: str, lo: int, hi: int | None) -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < lo or (hi is not None and value > hi):
        raise ValueError(f"{name} must be an integer in {lo} .. {hi if hi is not None else 'any'}, not {value!r}")
    return int(value)


def _need_gpu():
    if not torch.cuda.is_available():
        raise ops._lib.VFError("variantformer_amd.enrichment needs a GPU (no CPU fallback)")


def _pairs(annotations):
    """(gene id, iterable of terms) pairs out of a dict or a two-column frame."""
    if isinstance(annotations, dict):
        return list(annotations.items())
    if hasattr(annotations, "columns") and hasattr(annotations, "itertuples"):
        if len(annotations.columns) != 2:
            raise ValueError(f"an annotation frame has two columns, gene id and its list of terms, not {len(annotations.columns)}")
        return list(annotations.itertuples(index=False, name=None))
    raise TypeError(f"annotations must be a dict gene id -> terms or a two-column frame, not {type(annotations).__name__}")


def membership(annotations, universe, min_size: int = 1, max_size: int | None = None) -> Membership:
    """The annotation as term-major CSR over `universe`.  annotations: a dict, or a two-column frame, gene id -> list of terms
    (what the notebook's gene_go_annotations.parquet holds; a single string is one term, None / NaN no term).  universe: the
    gene ids of the rows, each once.  A gene outside the universe is dropped, a term listed twice by a gene counts once, a gene
    that appears twice in the frame has its lists united.  Terms with fewer than min_size or more than max_size genes in the
    universe are dropped.  The kept terms are in sorted order of their names (by str where the names do not compare).  Returns
    a Membership; everything is on the host."""
    min_size = _int_in(min_size, "min_size", 0, None)
    max_size = None if max_size is None else _int_in(max_size, "max_size", min_size, None)
    if isinstance(universe, (str, bytes)) or not hasattr(universe, "__iter__"):
        raise TypeError(f"universe must be a sequence of gene ids, not {type(universe).__name__}")
    universe = list(universe)
    if len(universe) > MAX_N:
        raise ValueError(f"universe holds {len(universe)} genes, above 2^24")
    row = {g: i for i, g in enumerate(universe)}
    if len(row) != len(universe):
        raise ValueError("universe names a gene twice")
    members = {}
    for gene_id, terms in _pairs(annotations):
        i = row.get(gene_id)
        if i is None or terms is None or (isinstance(terms, float) and terms != terms):
            continue
        if isinstance(terms, (str, bytes)):
            terms = (terms,)
        if not hasattr(terms, "__iter__"):
            raise TypeError(f"the terms of gene {gene_id!r} must be a list, not {type(terms).__name__}")
        for t in terms:
            members.setdefault(t, set()).add(i)
    hi = len(universe) if max_size is None else max_size
    kept = [t for t, s in members.items() if min_size <= len(s) <= hi]
    try:
        kept.sort()
    except TypeError:
        kept.sort(key=str)
    termptr = np.zeros(len(kept) + 1, dtype=np.int64)
    termptr[1:] = np.cumsum([len(members[t]) for t in kept], dtype=np.int64)
    gene = np.fromiter((i for t in kept for i in sorted(members[t])), dtype=np.int32, count=int(termptr[-1]))
    return Membership(termptr, gene, kept, len(universe))


def _check_membership(m) -> Membership:
    if not isinstance(m, Membership):
        raise TypeError(f"membership must be what enrichment.membership returned, not {type(m).__name__}")
    termptr, gene = np.asarray(m.termptr), np.asarray(m.gene)
    G = _int_in(m.genes, "membership.genes", 0, MAX_N)
    if termptr.ndim != 1 or termptr.shape[0] != len(m.terms) + 1 or termptr.dtype != np.int64:
        raise ValueError(f"membership.termptr must be int64 [terms + 1 = {len(m.terms) + 1}], not {termptr.dtype} {tuple(termptr.shape)}")
    if gene.ndim != 1 or gene.dtype != np.int32:
        raise ValueError(f"membership.gene must be int32 [entries], not {gene.dtype} {tuple(gene.shape)}")
    if termptr[0] != 0 or termptr[-1] != gene.shape[0] or (np.diff(termptr) < 0).any():
        raise ValueError("membership.termptr must rise from 0 to the number of entries")
    if gene.size and (gene.min() < 0 or gene.max() >= G):
        raise ValueError(f"membership.gene must hold rows of the universe, 0 .. {G - 1}")
    return Membership(termptr, gene, list(m.terms), G)


def _check_labels(labels, G: int, n_clusters):
    """(labels int32 numpy [G], k): integers; 0 .. k - 1 name a cluster, anything else no cluster."""
    if isinstance(labels, torch.Tensor):
        labels = labels.detach().cpu().numpy()
    if not isinstance(labels, np.ndarray):
        raise TypeError(f"labels must be a numpy array or a torch tensor of integers, not {type(labels).__name__}")
    if labels.ndim != 1 or labels.shape[0] != G:
        raise ValueError(f"labels must hold one integer per gene of the universe, [{G}], not {tuple(labels.shape)}")
    if labels.dtype == np.bool_ or not np.issubdtype(labels.dtype, np.integer):
        raise ValueError(f"labels must be integers, not {labels.dtype}")
    if G and (labels.min() < np.iinfo(np.int32).min or labels.max() > np.iinfo(np.int32).max):
        raise ValueError("labels must fit an int32")
    if n_clusters is None:
        top = int(labels.max()) if G else -1
        if top < 0:
            raise ValueError("labels name no cluster: every value is negative")
        if top >= MAX_K:
            raise ValueError(f"n_clusters = the largest label + 1 must be an integer in 1 .. {MAX_K}, not {top + 1}")
        k = top + 1
    else:
        k = _int_in(n_clusters, "n_clusters", 1, MAX_K)
    return np.ascontiguousarray(labels, dtype=np.int32), k


def _alternative(alternative) -> int:
    if alternative not in ALTERNATIVES:
        raise ValueError(f"alternative must be one of {ALTERNATIVES}, not {alternative!r}")
    return ALTERNATIVES.index(alternative)


def log_factorials(N: int) -> np.ndarray:
    """fp64 [N + 1]: lgamma(i + 1), by math.lgamma on the host -- the table vf_hypergeom_tail reads."""
    N = _int_in(N, "N", 0, MAX_N)
    return np.fromiter((math.lgamma(i + 1.0) for i in range(N + 1)), dtype=np.float64, count=N + 1)


def _hypergeom(labels: np.ndarray, k: int, m: Membership, alternative: int):
    """The device part: (count, size, csize, log_p, tail, steps) as tensors on the device."""
    dev = torch.device("cuda", torch.cuda.current_device())
    T, G = len(m.terms), m.genes
    termptr, gene = torch.from_numpy(m.termptr).to(dev), torch.from_numpy(m.gene).to(dev)
    lab = torch.from_numpy(labels).to(dev)
    count = torch.empty((T, k), dtype=torch.int32, device=dev)
    size = torch.empty(T, dtype=torch.int32, device=dev)
    ops.enrich_counts(termptr, gene, lab, k, count=count, size=size, family="enrich")
    # the cluster sizes: the same entry over the one term that lists every gene
    every = torch.arange(G, dtype=torch.int32, device=dev)
    whole = torch.tensor([0, G], dtype=torch.int64, device=dev)
    csize = torch.empty((1, k), dtype=torch.int32, device=dev)
    ops.enrich_counts(whole, every, lab, k, count=csize, size=torch.empty(1, dtype=torch.int32, device=dev), family="enrich")
    csize = csize[0]
    logfact = torch.from_numpy(log_factorials(G)).to(dev)
    log_p = torch.empty((T, k), dtype=torch.float64, device=dev)
    tail = torch.empty((T, k), dtype=torch.float64, device=dev)
    steps = torch.empty((T, k), dtype=torch.int32, device=dev)
    ops.hypergeom_tail(count, size, csize, G, logfact, alternative, log_p=log_p, tail=tail, steps=steps, family="enrich")
    return count, size, csize, log_p, tail, steps


def hypergeom(labels, membership: Membership, alternative: str = "greater", n_clusters: int | None = None, return_steps: bool = False):
    """The hypergeometric test of every (term, cluster) cell.  labels: one integer per gene of the universe, 0 .. k - 1 naming
    its cluster, any other value (-1) no cluster: such a gene stays in the universe; k = n_clusters, by default the largest
    label + 1 (at most 4096).  alternative "greater" tests over-representation, P[X >= count]; "less" P[X <= count].  Returns a
    dict of numpy arrays: count int32 [T, k], term_size int32 [T], cluster_size int32 [k], log_p and p = exp(log_p) fp64 [T, k];
    return_steps=True adds tail fp64 and steps int32 [T, k], the device's sums and their lengths."""
    m = _check_membership(membership)
    alt = _alternative(alternative)
    labels, k = _check_labels(labels, m.genes, n_clusters)
    _need_gpu()
    count, size, csize, log_p, tail, steps = _hypergeom(labels, k, m, alt)
    out = {"count": count.cpu().numpy(), "term_size": size.cpu().numpy(), "cluster_size": csize.cpu().numpy(),
           "log_p": log_p.cpu().numpy(), "p": torch.exp(log_p).cpu().numpy()}
    if return_steps:
        out["tail"], out["steps"] = tail.cpu().numpy(), steps.cpu().numpy()
    return out


def _bh(p: torch.Tensor) -> torch.Tensor:
    """Benjamini-Hochberg q of the fp64 tensor p over all its cells, on p's device: scipy.stats.false_discovery_control(ps,
    method="bh") operation for operation -- sort, ps *= m / arange(1, m + 1), a running minimum from the largest down, the
    order undone, a clip to [0, 1]."""
    assert p.dtype == torch.float64
    ps = p.reshape(-1)
    m = ps.shape[0]
    if m == 0:
        return p.clone()
    ordered, order = torch.sort(ps, stable=True)
    i = torch.arange(1, m + 1, dtype=torch.float64, device=p.device)
    ordered = ordered * (torch.full_like(i, float(m)) / i)             # a true division: `m / i` would be m * reciprocal(i)
    ordered = torch.flip(torch.cummin(torch.flip(ordered, (0,)), 0).values, (0,))
    q = torch.empty_like(ordered)
    q[order] = ordered
    return q.clamp(0.0, 1.0).reshape(p.shape)


def enrich(labels, annotations, universe=None, fdr: float = 0.05, alternative: str = "greater", n_clusters: int | None = None,
           min_size: int = 5, max_size: int | None = 500, cluster_names=None):
    """Which terms are over-represented ("greater") in which cluster.  annotations and universe as in `membership` (or a
    finished Membership, universe=None); labels, alternative and n_clusters as in `hypergeom`; min_size / max_size filter the
    terms by their size in the universe.  Returns hypergeom's dict plus
      terms     the names of the T tested terms;
      fold      fp64 [T, k]: (count / cluster_size) / (term_size / N), NaN or Inf where a size is 0;
      q         fp64 [T, k]: Benjamini-Hochberg over all T * k tested cells;
      frame     a pandas frame of the cells with q <= fdr, sorted by q (then p, term, cluster): cluster, term, count,
                term_size, cluster_size, fold, log_p, p, q.  cluster_names, a sequence of k names, replaces the cluster numbers."""
    import pandas as pd
    if isinstance(fdr, bool) or not isinstance(fdr, (int, float, np.integer, np.floating)) or not 0 < fdr <= 1:
        raise ValueError(f"fdr must be a number in (0, 1], not {fdr!r}")
    alt = _alternative(alternative)
    if isinstance(annotations, Membership):
        if universe is not None:
            raise ValueError("a finished Membership carries its universe: pass universe=None")
        m = _check_membership(annotations)
    else:
        if universe is None:
            raise ValueError("universe is needed to read an annotation: the gene ids of the rows that labels describes")
        m = membership(annotations, universe, min_size=min_size, max_size=max_size)
    labels, k = _check_labels(labels, m.genes, n_clusters)
    if cluster_names is not None and len(cluster_names) != k:
        raise ValueError(f"cluster_names must name the {k} clusters, not {len(cluster_names)}")
    _need_gpu()
    count, size, csize, log_p, _, _ = _hypergeom(labels, k, m, alt)
    p = torch.exp(log_p)
    fold = (count.double() / csize.double()[None, :]) / (size.double()[:, None] / float(m.genes))
    q = _bh(p)
    out = {"terms": m.terms, "count": count.cpu().numpy(), "term_size": size.cpu().numpy(), "cluster_size": csize.cpu().numpy(),
           "log_p": log_p.cpu().numpy(), "p": p.cpu().numpy(), "fold": fold.cpu().numpy(), "q": q.cpu().numpy()}
    t, c = np.nonzero(out["q"] <= fdr)
    order = np.lexsort((c, t, out["log_p"][t, c], out["q"][t, c]))
    t, c = t[order], c[order]
    names = np.arange(k) if cluster_names is None else np.array(list(cluster_names), dtype=object)
    terms = np.empty(len(m.terms), dtype=object)
    terms[:] = m.terms
    out["frame"] = pd.DataFrame({"cluster": names[c], "term": terms[t], "count": out["count"][t, c], "term_size": out["term_size"][t],
                                 "cluster_size": out["cluster_size"][c], "fold": out["fold"][t, c], "log_p": out["log_p"][t, c],
                                 "p": out["p"][t, c], "q": out["q"][t, c]})
    return out
