"""The plain-Python twin of the error-profile kernel, written from the definition on top of
cons_utils.row_reference, for the error-profile tests: per job the vote table, the members' eight counts and the job's
q / subst / ins / hp tables (profile_reference, a drop-in for errors.profile), and the pieces the tests ask about one by
one (member_profile, draft_runs)."""
import numpy as np

from cons_utils import code, pair_limit, reduce_rows, row_reference

MEMBER_WORDS, Q_BINS, JOB_WORDS = 8, 64, 274
Q, SUBST, INS, HP = 0, 192, 212, 218


def draft_runs(draft):
    """The runs of a draft (bytes): (s, r, b) for every maximal stretch [s, s + r) of one code b <= 3."""
    runs, p, m = [], 0, len(draft)
    while p < m:
        b, s = code(draft[p]), p
        while p < m and code(draft[p]) == b:
            p += 1
        if b <= 3:
            runs.append((s, p - s, b))
    return runs


def phred_bin(byte):
    return 0 if byte < 33 else min(byte - 33, 63)


def member_profile(draft, row, qual):
    """(words[8], tables[274], consumed) of one member within its limit: its row (m + 1 words) over the draft (bytes) and
    its quality bytes.  consumed = the sum of c_p, the read's length for an unclipped member."""
    m = len(draft)
    t = [0] * JOB_WORDS
    match = sub = dele = other = events = bases = 0
    sym = [w & 7 for w in row]
    length = [(w >> 3) & 255 for w in row]
    kept = [[(w >> (11 + 3 * i)) & 7 for i in range(min(L, 4))] for w, L in zip(row, length)]
    clipped = any(L == 255 for L in length)
    rp, qcount = 0, []                                        # qcount: (bin, kind) per read byte the row accounts for
    for p in range(m + 1):
        L = length[p]
        if L:
            events += 1
            bases += L
            for c in kept[p]:
                t[INS + c] += 1
            t[INS + 5] += L - len(kept[p])
        qcount += [(rp + i, 2) for i in range(L)]
        rp += L                                               # now rp(p)
        if p == m:
            break
        dc = code(draft[p])
        if sym[p] == 5:
            dele += 1
            cls = "del"
        elif sym[p] <= 3 and dc <= 3:
            cls = "match" if sym[p] == dc else "sub"
            match, sub = match + (cls == "match"), sub + (cls == "sub")
        else:
            other += 1
            cls = "other"
        if dc <= 3 and (sym[p] <= 3 or sym[p] == 5):
            t[SUBST + dc * 5 + (4 if sym[p] == 5 else sym[p])] += 1
        if cls != "del":
            qcount.append((rp, 0 if cls == "match" else 1))
            rp += 1
    if not clipped:
        assert rp == len(qual), (rp, len(qual))
        for at, kind in qcount:
            t[Q + phred_bin(qual[at]) * 3 + kind] += 1
    for s, r, b in draft_runs(draft):
        obs = sum(sym[p] == b for p in range(s, s + r)) + sum(c == b for p in range(s, s + r + 1) for c in kept[p])
        t[HP + (min(r, 8) - 1) * 7 + max(-3, min(3, obs - r)) + 3] += 1
    return [match, sub, dele, other, events, bases, int(clipped), 0], t, rp


def profile_reference(reads, quals, ks, jobs, kernel_ms=None):
    """errors.profile without a device: per job (vote table, aligned, member counts [n, 8], tables [274])."""
    out = []
    for draft, r0, n in jobs:
        m = len(reads[draft])
        words = np.zeros((n, MEMBER_WORDS), dtype=np.uint32)
        tables = np.zeros(JOB_WORDS, dtype=np.uint32)
        rows = []
        for i in range(n):
            r = r0 + i
            d, row = row_reference(reads[draft], reads[r], pair_limit(ks[draft], ks[r]))
            if d < 0:
                continue
            rows.append(row)
            w, t, _ = member_profile(reads[draft], row, quals[r])
            words[i] = w
            tables += np.array(t, dtype=np.uint32)
        out.append((reduce_rows(np.array(rows, dtype=np.uint32).reshape(len(rows), m + 1), m), len(rows), words, tables))
    return out
