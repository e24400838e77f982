"""The plain-Python twin of the consensus kernels, written from the definition, for the consensus
tests: the pileup row of a read over a draft from the full NW matrix and the fixed walk (row_reference), the vote tables
of a batch of jobs (votes_reference, a drop-in for consensus.votes) and the polishing rounds (consensus_reference)."""
import numpy as np

from specimux_amd import consensus

MAX_INS, VOTE_WORDS = 4, 26
NO_ROW = 0xFFFFFFFF


def code(byte):
    """0-3 = the bytes A C G T, 4 = any other byte."""
    return {65: 0, 67: 1, 71: 2, 84: 3}.get(byte, 4)


def nw_matrix(q, t):
    """D[i][j], (m + 1) x (n + 1): the edit distance of q[:i] and t[:j].  A row's left-to-right dependency
    D[i][j] = min(x[j], D[i][j-1] + 1) is a running minimum of x[j] - j."""
    qa, ta = np.frombuffer(q, dtype=np.uint8), np.frombuffer(t, dtype=np.uint8)
    idx = np.arange(len(t) + 1, dtype=np.int32)
    D = np.empty((len(q) + 1, len(t) + 1), dtype=np.int32)
    D[0] = idx
    for i in range(1, len(q) + 1):
        x = np.empty(len(t) + 1, dtype=np.int32)
        x[0] = i
        np.minimum(D[i - 1, :-1] + (ta != qa[i - 1]), D[i - 1, 1:] + 1, out=x[1:])
        D[i] = np.minimum.accumulate(x - idx) + idx
    return D


def row_reference(draft, read, k):
    """(distance, row) of `read` (bytes) over `draft` (bytes): the NW distance, or -1 above the limit k (k < 0: none),
    and the m + 1 row words -- all 0xFFFFFFFF above the limit.  The walk starts at (m, n): diagonal if
    D[i-1][j-1] + (q[i-1] != t[j-1]) == D[i][j], else up if D[i-1][j] + 1 == D[i][j] (a deletion in the read), else
    left (an insertion)."""
    m, n = len(draft), len(read)
    D = nw_matrix(draft, read)
    D = D.tolist() if D.size < 1 << 22 else D          # lists walk faster; a large matrix stays an array
    d = int(D[m][n])
    if 0 <= k < d:
        return -1, [NO_ROW] * (m + 1)
    sym = [7] * (m + 1)
    ins = [[] for _ in range(m + 1)]           # the inserted codes before position p, last first
    i, j = m, n
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i - 1][j - 1] + (draft[i - 1] != read[j - 1]) == D[i][j]:
            sym[i - 1] = code(read[j - 1])
            i, j = i - 1, j - 1
        elif i > 0 and D[i - 1][j] + 1 == D[i][j]:
            sym[i - 1] = 5
            i -= 1
        else:
            ins[i].append(code(read[j - 1]))
            j -= 1
    row = []
    for p in range(m + 1):
        w = sym[p] | (min(len(ins[p]), 255) << 3)
        for s, c in enumerate(ins[p][::-1][:MAX_INS]):
            w |= c << (11 + 3 * s)
        row.append(w)
    return d, row


def pair_limit(kd, kr):
    return -1 if kd < 0 or kr < 0 else max(kd, kr)


def pileup_reference(reads, ks, jobs):
    """What smx_cons_pileup returns: (rows, dist), job after job."""
    rows, dist = [], []
    for draft, r0, n in jobs:
        for r in range(r0, r0 + n):
            d, row = row_reference(reads[draft], reads[r], pair_limit(ks[draft], ks[r]))
            dist.append(d)
            rows += row
    return np.array(rows, dtype=np.uint32), np.array(dist, dtype=np.int32)


def reduce_rows(rows, m):
    """The (m + 1) x 26 vote table of rows (members x (m + 1) words, numpy) that all voted: per position sym[6], then
    ins[slot][code]; a read whose insertion before p has length L votes in slots 0 .. min(L, 4) - 1."""
    table = np.zeros((m + 1, VOTE_WORDS), dtype=np.uint32)
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1, m + 1)
    s = rows & 7
    for c in range(6):
        table[:, c] = (s == c).sum(axis=0)
    length = (rows >> 3) & 255
    for slot in range(MAX_INS):
        has = length > slot
        codes = (rows >> (11 + 3 * slot)) & 7
        for c in range(5):
            table[:, 6 + 5 * slot + c] = (has & (codes == c)).sum(axis=0)
    return table


def votes_reference(reads, ks, jobs, kernel_ms=None):
    """consensus.votes without a device: per job its vote table and the number of members within their limit."""
    tables, aligned = [], []
    for draft, r0, n in jobs:
        m = len(reads[draft])
        rows = []
        for r in range(r0, r0 + n):
            d, row = row_reference(reads[draft], reads[r], pair_limit(ks[draft], ks[r]))
            if d >= 0:
                rows.append(row)
        tables.append(reduce_rows(np.array(rows, dtype=np.uint32).reshape(len(rows), m + 1), m))
        aligned.append(len(rows))
    return tables, aligned


def consensus_reference(draft, reads, rounds=3, k=-1, min_aligned=1, votes_fn=votes_reference):
    """The polishing rounds over one group of reads (str) from a draft that need not be one of them: every read votes
    under the limit k in every round (k < 0: none); stops as the tool does.  Returns the consensus."""
    raw = [r.encode("latin-1") for r in reads]
    for _ in range(rounds):
        tables, aligned = votes_fn(raw + [draft.encode("latin-1")], [k] * (len(raw) + 1), [(len(raw), 0, len(raw))])
        if aligned[0] < min_aligned:
            break
        new = consensus.call_consensus(draft, tables[0], aligned[0])
        if not new or new == draft:
            break
        draft = new
    return draft
