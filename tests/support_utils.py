"""The plain-Python twin of the resampling kernel, written from the definition on top of
cons_utils.row_reference, for the support tests: per replicate the seven counts of every column over its voters' pileup
rows and the rule as §20 writes it (resample_reference, a drop-in for support.resample), and a replicate's full 26-word
vote table for the tests that hand it to consensus.call_consensus (replicate_table)."""
import numpy as np

from cons_utils import pair_limit, reduce_rows, row_reference
from specimux_amd.support import REPLICATES, JobSupport

CODES = {65: 0, 67: 1, 71: 2, 84: 3}       # the bytes A C G T; any other byte is 4


def job_rows(reads, ks, job):
    """(distances, rows) of one job's members over its draft: n distances, n x (m + 1) words (0xFFFFFFFF rows above the limit)."""
    draft, r0, n = job
    pairs = [row_reference(reads[draft], reads[r], pair_limit(ks[draft], ks[r])) for r in range(r0, r0 + n)]
    m = len(reads[draft])
    return [d for d, _ in pairs], np.array([row for _, row in pairs], dtype=np.uint32).reshape(n, m + 1)


def replicate_members(dists, mask_words, b):
    """The voters of replicate b: the members whose mask word has bit b and whose distance is within the limit."""
    return [i for i, d in enumerate(dists) if d >= 0 and (int(mask_words[i]) >> b) & 1]


def replicate_table(rows, dists, mask_words, b):
    """((m + 1) x 26 vote table, n_b) of replicate b."""
    who = replicate_members(dists, mask_words, b)
    m = rows.shape[1] - 1
    return reduce_rows(rows[who].reshape(len(who), m + 1), m), len(who)


def keeps_reference(draft, rows, dists, mask_words):
    """(keep, n_b): keep[b][p] for the 64 replicates and the columns 0..m, and the replicates' voters.  Over the voters of
    replicate b at column p: a[0..3] the row words whose bits 0-2 are 0..3, del those with 5, ins those whose bits 3-10 are
    not zero; b keeps p iff  !(2 ins > n_b) && (p == m || (!(2 del > n_b) && (max a == 0 || (dc < 4 && a[dc] == max a))))."""
    n, m = rows.shape[0], rows.shape[1] - 1
    member = np.array([[d >= 0 and (int(w) >> b) & 1 for d, w in zip(dists, mask_words)] for b in range(REPLICATES)],
                      dtype=np.int64).reshape(REPLICATES, n)
    sym, has_ins = (rows & 7).astype(np.int64), (((rows >> 3) & 255) != 0).astype(np.int64)
    a = np.stack([member @ (sym == x) for x in range(4)])                 # 4 x 64 x (m + 1)
    dele, ins, n_b = member @ (sym == 5), member @ has_ins, member.sum(axis=1)
    top = a.max(axis=0)
    own = np.full((REPLICATES, m + 1), -1, dtype=np.int64)               # a[dc]; -1 where the draft's byte is no base
    for p, byte in enumerate(draft):
        if byte in CODES:
            own[:, p] = a[CODES[byte], :, p]
    base_ok = ~(2 * dele > n_b[:, None]) & ((top == 0) | (own == top))
    last = np.arange(m + 1) == m
    return ~(2 * ins > n_b[:, None]) & (last[None, :] | base_ok), n_b


def resample_reference(reads, ks, jobs, masks, kernel_ms=None):
    """support.resample without a device."""
    masks = np.asarray(masks, dtype=np.uint64)
    n_levels = masks.shape[0]
    out, at = [], 0
    weights = [1 << b for b in range(REPLICATES)]
    for job in jobs:
        draft, _r0, n = job
        m = len(reads[draft])
        dists, rows = job_rows(reads, ks, job)
        voted = rows[[i for i, d in enumerate(dists) if d >= 0]]
        agree = np.zeros((n_levels, m + 1), dtype=np.uint64)
        sub = np.zeros((n_levels, REPLICATES), dtype=np.uint32)
        for l in range(n_levels):
            keep, n_b = keeps_reference(reads[draft], rows, dists, masks[l, at:at + n])
            agree[l] = [sum(w for w, k in zip(weights, keep[:, p]) if k) for p in range(m + 1)]
            sub[l] = n_b
        out.append(JobSupport(reduce_rows(voted.reshape(len(voted), m + 1), m), len(voted), agree, sub))
        at += n
    return out
