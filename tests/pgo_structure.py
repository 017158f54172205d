"""The pose graph's solver structure, restated from the host side of myslam_pose_graph_optimize (csrc/pgo.hip, "structure" and the run
cutting that follows it), so that a test can state which regime a graph drives the library into and assert it.

  separators  repeatedly, the key-frame on the most off-chain edges (edges between free non-separator key-frames more than one chain
              position apart) becomes a separator, the latest key-frame on ties, until no off-chain edge is left; more than
              PG_MAXS_BIG of them and the call is refused (MYSLAM_ERR_UNSUPPORTED)
  budget      PG_MAXS when the natural separators fit the fast path, PG_MAXS_BIG otherwise
  cuts        every chain run longer than lmax = max(16, ceil(sqrt(11 nT))) is cut into equal parts by extra separators; when the
              cuts do not fit the budget, lmax doubles until they do
  path        "fast" (k_pg_schur<false>: at most PG_MAXS separators in all), "general" (k_pg_schur<true>) or "refused"
"""
import math
from dataclasses import dataclass

import numpy as np

PG_MAXS = 96
PG_MAXS_BIG = 1024


@dataclass
class PgStructure:
    natural: int          # separators before the cuts (PG_MAXS_BIG + 1 when refused: the library stops counting there)
    cuts: int             # separators added by cutting chain runs
    path: str             # "fast" | "general" | "refused"
    longest_run: int      # the longest chain run the block-tridiagonal sweep walks
    n_chain: int          # free non-separator key-frames after the cuts
    doublings: int        # times lmax doubled before the cuts fit the budget
    chosen: tuple = ()    # the natural separators in the order they were chosen

    @property
    def separators(self):
        return self.natural + self.cuts


def _chain_positions(free):
    return np.where(free, np.cumsum(free) - 1, -1)


def _links(tpos, nT, e0, e1):
    """link[t]: an edge joins chain positions t-1 and t (the library's chain_links)"""
    a, b = tpos[e0], tpos[e1]
    m = (a >= 0) & (b >= 0)
    link = np.zeros(nT + 1, bool)
    link[np.maximum(a[m], b[m])] = True
    link[0] = False
    link[nT] = False
    return link


def _runs(link, nT):
    """chain runs as (start, length)"""
    out, s0 = [], 0
    while s0 < nT:
        e = s0 + 1
        while e < nT and link[e]:
            e += 1
        out.append((s0, e - s0))
        s0 = e
    return out


def pg_structure(n, fixed, e0, e1):
    fx = np.asarray(fixed).astype(bool) if fixed is not None else np.zeros(n, bool)
    e0 = np.asarray(e0, np.int64); e1 = np.asarray(e1, np.int64)
    inS = np.zeros(n, bool)
    nS, chosen = 0, []
    while True:
        tpos = _chain_positions(~fx & ~inS)
        a, b = tpos[e0], tpos[e1]
        m = (a >= 0) & (b >= 0) & (np.abs(a - b) > 1)
        if not m.any():
            break
        deg = np.bincount(e0[m], minlength=n) + np.bincount(e1[m], minlength=n)
        best = n - 1 - int(np.argmax(deg[::-1]))                      # the most off-chain edges, latest on ties
        inS[best] = True
        chosen.append(best)
        nS += 1
        if nS > PG_MAXS_BIG:
            return PgStructure(nS, 0, "refused", 0, 0, 0, tuple(chosen))
    natural = nS
    budget = PG_MAXS if nS <= PG_MAXS else PG_MAXS_BIG
    free = ~fx & ~inS
    nT = int(free.sum())
    tvert = np.flatnonzero(free)
    runs = _runs(_links(_chain_positions(free), nT, e0, e1), nT)
    lmax, doublings = max(16, int(math.ceil(math.sqrt(11.0 * nT)))), 0
    while True:
        cuts = []
        for s0, ln in runs:
            parts = (ln + 1 + lmax) // (lmax + 1)
            cuts += [s0 + i * ln // parts for i in range(1, parts)]
        if nS + len(cuts) > budget:
            if not cuts:
                return PgStructure(natural, 0, "refused", 0, nT, doublings, tuple(chosen))
            lmax *= 2; doublings += 1
            continue
        break
    inS[tvert[cuts]] = True
    nS += len(cuts)
    free = ~fx & ~inS
    nT = int(free.sum())
    runs = _runs(_links(_chain_positions(free), nT, e0, e1), nT)
    return PgStructure(natural, len(cuts), "general" if nS > PG_MAXS else "fast", max((ln for _, ln in runs), default=0), nT,
                       doublings, tuple(chosen))
