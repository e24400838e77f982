"""The plain-Python twin of the variant kernels, written from the definition on top of
cons_utils.row_reference, for the variants tests: the site rule over a vote table (sites_reference), every member's
allele at the kept sites as plane words (planes_reference), the link counts by plain loops over the members
(link_reference), and a drop-in for variants.phase (phase_reference)."""
import numpy as np

from cons_utils import pair_limit, reduce_rows, row_reference
from specimux_amd.variants import JobPhase, Site

BASE_CODES = (0, 1, 2, 3, 5)               # A C G T deletion: the symbols a base site ranges over ("other", 4, is ignored)


def qualifies(n_minor, aligned, min_permille, min_reads):
    return n_minor >= min_reads and 1000 * n_minor >= min_permille * aligned


def candidates(table, aligned, m):
    """Every candidate of an (m + 1) x 26 vote table in the order (p, insertion before base)."""
    rows = np.asarray(table).tolist()
    for p in range(m + 1):
        present = sum(rows[p][6:11])
        absent = aligned - present
        if present <= absent:                                  # the smaller is minor; `present` on a tie
            yield Site(p, 1, 0, 1, absent, present)
        else:
            yield Site(p, 1, 1, 0, present, absent)
        if p < m:
            order = sorted(BASE_CODES, key=lambda c: (-rows[p][c], c))   # most votes first, ties to the lower code
            yield Site(p, 0, order[0], order[1], rows[p][order[0]], rows[p][order[1]])


def sites_reference(table, aligned, m, n, min_permille, min_reads, max_sites):
    """(kept sites, n_qualified) of one job; a job without members has none."""
    if n == 0:
        return [], 0
    good = [s for s in candidates(table, aligned, m) if qualifies(s.n_minor, aligned, min_permille, min_reads)]
    return good[:max_sites], len(good)


def classify(word, site):
    """1 = the site's minor allele, 2 = its major allele, 0 = neither."""
    code = int(((word >> 3) & 255) != 0) if site.kind else word & 7
    return 1 if code == site.minor else 2 if code == site.major else 0


def classes_reference(rows, dists, sites):
    """classes[s][i] of member i at site s; a member above its limit has neither allele anywhere."""
    return [[classify(row[site.pos], site) if d >= 0 else 0 for row, d in zip(rows, dists)] for site in sites]


def planes_reference(classes, n, max_sites):
    """max_sites x 2 x ceil(n / 64) uint64: bit i & 63 of word i >> 6 of plane [s][0] / [s][1] for a minor / major member i."""
    planes = np.zeros((max_sites, 2, (n + 63) // 64), dtype=np.uint64)
    for s, cls in enumerate(classes):
        for i, c in enumerate(cls):
            if c:
                planes[s, c - 1, i >> 6] |= np.uint64(1 << (i & 63))
    return planes


def link_reference(classes, max_sites):
    """max_sites x max_sites x 4 uint32: for s < t the members that are (minor, minor), (minor, major), (major, minor),
    (major, major) at (s, t); zero elsewhere."""
    link = np.zeros((max_sites, max_sites, 4), dtype=np.uint32)
    slot = {(1, 1): 0, (1, 2): 1, (2, 1): 2, (2, 2): 3}
    for s in range(len(classes)):
        for t in range(s + 1, len(classes)):
            for a, b in zip(classes[s], classes[t]):
                if a and b:
                    link[s, t, slot[a, b]] += 1
    return link


def phase_reference(reads, ks, jobs, min_permille, min_reads, max_sites, kernel_ms=None):
    """variants.phase without a device."""
    out = []
    for draft, r0, n in jobs:
        m = len(reads[draft])
        pairs = [row_reference(reads[draft], reads[r], pair_limit(ks[draft], ks[r])) for r in range(r0, r0 + n)]
        dists, rows = [d for d, _ in pairs], [row for _, row in pairs]
        voted = [row for d, row in pairs if d >= 0]
        table = reduce_rows(np.array(voted, dtype=np.uint32).reshape(len(voted), m + 1), m)
        sites, n_qualified = sites_reference(table, len(voted), m, n, min_permille, min_reads, max_sites)
        classes = classes_reference(rows, dists, sites)
        out.append(JobPhase(table, len(voted), sites, n_qualified, planes_reference(classes, n, max_sites),
                            link_reference(classes, max_sites)))
    return out
