#!/usr/bin/env python3
"""specimux-variants: split the clusters of specimux-consensus into haplotypes by linked sites.  (The reference has no
such tool.)

specimux-clusters separates sequences only when they differ by more than the read noise, so two ITS copies of a
dikaryon, two alleles or a sister species that differ at a few positions share one cluster, and specimux-consensus calls
the majority at every column.  This tool runs consensus.consensus_files as it stands and then aligns the reads of every
polished cluster to the cluster's final consensus once more, in one smx_cons_phase call per planned device call (HIP
kernels smx_cons.hip and smx_phase.hip; there is no CPU path).  On the device the call finds the columns where a second
allele has at least `--min-site-share` of the aligned reads (and `--min-cluster-size` reads), every read's allele at
those columns, and for every pair of columns how often the alleles go together.  The decisions are made on the host
from those integers:

  linked     two sites whose alleles are correlated across the reads: r^2 >= `--min-r2` over the reads with a call at both
  accepted   a site linked to at least one other; or a substitution whose minor allele alone has `--single-share` of the
             aligned reads.  An unlinked indel -- the systematic error of a homopolymer run -- is never accepted
  haplotype  a signature (major / minor at every accepted site) carried by at least `--min-cluster-size` reads and
             `--min-hap-share` of the aligned reads; every other read joins the one haplotype nearest to its calls, a read
             that ties stays unassigned.  Fewer than two haplotypes: the cluster is `single` and is reported as
             specimux-consensus reports it

Each haplotype's reads are then polished (consensus.polish) from the cluster's consensus as draft 0.

    python -m specimux_amd.variants --fastq full/POOL/SPECIMEN.fastq --fasta OUT.fasta [--report R.tsv] [--json R.json]
        [--sites S.tsv] [--min-site-share 0.15] [--min-r2 0.5] [--single-share 0.30] [--min-hap-share 0.10]
        [--max-sites 32] [specimux-consensus' options]
    python -m specimux_amd.variants --run-dir OUT [--level pool|primer-pair] [...]

--json keeps the layout of specimux-consensus --json (haplotypes are entries of `clusters`, with `parent` and `sites`), so
specimux-crosstalk --consensus and specimux-identify --consensus read it as it is.  One GPU."""
import argparse
import json
import logging
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import calls, clusters, consensus, specimine

Job = consensus.Job
VOTE_WORDS = consensus.VOTE_WORDS
MAX_SITES = 64                             # smx.h: SMX_CONS_MAX_SITES
ALLELES = "ACGT?-"                         # kind 0: the row's codes 0-3 and 5


class Site(NamedTuple):
    """One kept site of a job (smx.h: smx_cons_site)."""
    pos: int
    kind: int                              # 0 = the base at pos, 1 = the insertion before pos
    major: int
    minor: int
    n_major: int
    n_minor: int


class JobPhase(NamedTuple):
    """What one smx_cons_phase call returns for one job."""
    table: np.ndarray                      # (m + 1) x 26 votes, as consensus.votes returns them
    aligned: int
    sites: List[Site]                      # the kept sites, at most max_sites
    n_qualified: int
    planes: np.ndarray                     # max_sites x 2 x ceil(n / 64) uint64: [site][0 = minor | 1 = major][word]
    link: np.ndarray                       # max_sites x max_sites x 4 uint32: [s][t] = n11, n10, n01, n00 for s < t


def build_parser() -> argparse.ArgumentParser:
    parser = consensus.build_parser()
    parser.description = "Split the clusters of each specimen into haplotypes by linked variant sites."
    parser.add_argument("--min-site-share", type=float, default=0.15,
                        help="Smallest share of the aligned reads the second allele of a column needs to be a site "
                             "(default: 0.15)")
    parser.add_argument("--min-r2", type=float, default=0.5,
                        help="Smallest squared correlation of two sites' alleles across the reads that links them (default: 0.5)")
    parser.add_argument("--single-share", type=float, default=0.30,
                        help="Minor share from which a substitution is accepted without a linked partner (default: 0.30)")
    parser.add_argument("--min-hap-share", type=float, default=0.10,
                        help="Smallest share of the aligned reads that carry a signature exactly for it to be a haplotype "
                             "(default: 0.10)")
    parser.add_argument("--max-sites", type=int, default=32,
                        help=f"Sites kept per cluster, 1..{MAX_SITES}: the first in sequence order (default: 32)")
    parser.add_argument("--sites", help="Write a TSV with one row per kept site")
    return parser


permille = specimine.permille


# ------------------------------------------------------------------------------------------------ the device call
def phase(reads: Sequence[bytes], ks: Sequence[int], jobs: Sequence[Job], min_permille: int, min_reads: int, max_sites: int,
          kernel_ms: Optional[list] = None) -> List[JobPhase]:
    """One smx_cons_phase call: per job what consensus.votes returns for it, its kept sites, its allele planes and its
    link table."""
    return [JobPhase(table, aligned, [Site(int(s["pos"]), int(s["kind"]), int(s["major"]), int(s["minor"]), int(s["n_major"]),
                                           int(s["n_minor"])) for s in kept], n_qualified, planes, link)
            for table, aligned, kept, n_qualified, planes, link
            in calls.cons_phase(reads, ks, jobs, min_permille, min_reads, max_sites, kernel_ms)]


# ------------------------------------------------------------------------------------------------ the decisions
def linked(n11: int, n10: int, n01: int, n00: int, min_cluster_size: int, r2_permille: int) -> bool:
    """Two sites are linked when their alleles are correlated over the reads with a call at both: every margin of the
    2 x 2 table is positive, the table holds at least min_cluster_size reads, and r^2 = (n11 n00 - n10 n01)^2 / (a b c d) is
    at least r2_permille / 1000.  The sign is not used: at 50/50 which allele is called minor is arbitrary."""
    a, b, c, d = n11 + n10, n01 + n00, n11 + n01, n10 + n00
    if min(a, b, c, d) <= 0 or a + b < min_cluster_size:
        return False
    return 1000 * (n11 * n00 - n10 * n01) ** 2 >= r2_permille * a * b * c * d


def is_substitution(site: Site) -> bool:
    return site.kind == 0 and site.major < 4 and site.minor < 4


def accept_sites(sites: Sequence[Site], link, aligned: int, min_cluster_size: int, r2_permille: int,
                 single_permille: int) -> Tuple[List[List[int]], List[bool]]:
    """Per kept site its linked partners and whether it is accepted: linked to at least one other site, or a substitution
    whose minor allele has single_permille of `aligned`.  An unlinked indel is never accepted."""
    n = len(sites)
    partners: List[List[int]] = [[] for _ in range(n)]
    for s in range(n):
        for t in range(s + 1, n):
            if linked(*(int(x) for x in link[s][t]), min_cluster_size, r2_permille):
                partners[s].append(t)
                partners[t].append(s)
    accepted = [bool(partners[s]) or (is_substitution(sites[s]) and 1000 * sites[s].n_minor >= single_permille * aligned)
                for s in range(n)]
    return partners, accepted


def member_calls(planes, which: Sequence[int], n: int) -> List[Tuple[Optional[int], ...]]:
    """Per member its call at each of the sites `which`: 1 = minor, 0 = major, None = neither."""
    bits = [[sum(int(w) << (64 * i) for i, w in enumerate(planes[s][a])) for a in (0, 1)] for s in which]
    return [tuple(1 if (mi >> i) & 1 else 0 if (ma >> i) & 1 else None for mi, ma in bits) for i in range(n)]


def haplotypes(calls: Sequence[Tuple[Optional[int], ...]], aligned: int, min_cluster_size: int,
               hap_permille: int) -> Tuple[List[Tuple[Tuple[int, ...], List[int]]], List[int]]:
    """The haplotypes of a cluster from its members' calls at the accepted sites: (signature, members) largest first, ties
    by signature, and the members left unassigned.  A signature is a haplotype when at least min_cluster_size members and
    hap_permille of `aligned` carry it with a call at every site; every other member joins the one haplotype at the least
    Hamming distance over the sites where it has a call, and stays unassigned on a tie.  Without an accepted site there is
    nothing to tell the members apart: no haplotypes."""
    if not calls or not calls[0]:
        return [], list(range(len(calls)))
    exact: Dict[Tuple[int, ...], List[int]] = {}
    for i, c in enumerate(calls):
        if None not in c:
            exact.setdefault(c, []).append(i)
    members = {sig: list(who) for sig, who in exact.items()
               if len(who) >= min_cluster_size and 1000 * len(who) >= hap_permille * aligned}
    unassigned = []
    for i, c in enumerate(calls):
        if c in members:                                       # one of the haplotype's own: a call at every site
            continue
        dist = sorted((sum(1 for x, y in zip(c, sig) if x is not None and x != y), sig) for sig in members)
        if len(dist) == 1 or (len(dist) > 1 and dist[0][0] < dist[1][0]):
            members[dist[0][1]].append(i)
        else:
            unassigned.append(i)
    order = sorted(members, key=lambda sig: (-len(members[sig]), sig))
    return [(sig, sorted(members[sig])) for sig in order], unassigned


# ------------------------------------------------------------------------------------------------ the run
class Haplotype:
    """One haplotype of a split cluster."""
    def __init__(self, index: int, signature: Tuple[int, ...], members: List[int]):
        self.index, self.signature, self.members = index, signature, members
        self.seq, self.aligned, self.rounds, self.stop = "", 0, 0, "rounds"


class Phased:
    """What the phase call and the decisions made of one polished cluster."""
    def __init__(self, pc: consensus.Polished):
        self.pc = pc
        self.aligned = 0
        self.sites: List[Site] = []
        self.n_qualified = 0
        self.partners: List[List[int]] = []
        self.accepted: List[bool] = []
        self.haps: List[Haplotype] = []         # empty: the cluster is single
        self.unassigned = 0


def variants_files(paths: Sequence[str], args, adjacency_fn: Callable = clusters.adjacency,
                   votes_fn: Callable = consensus.votes, phase_fn: Callable = phase, kernel_ms: Optional[list] = None):
    """consensus.consensus_files over `paths`, then per planned device call one phase_fn call over the polished clusters
    and one consensus.polish over the haplotypes it finds.  Returns consensus' results and polished clusters, per polished
    cluster its Phased, and the summary extended by {"phase_calls", "split", "haplotypes"}."""
    budget = clusters.budget_bytes()
    results, polished, summary = consensus.consensus_files(paths, args.min_identity, args.max_reads, args.min_cluster_size,
                                                           args.minor_share, args.rounds, budget=budget,
                                                           adjacency_fn=adjacency_fn, votes_fn=votes_fn, kernel_ms=kernel_ms)
    phased: List[List[Phased]] = [[Phased(pc) for pc in pcs] for pcs in polished]
    summary = dict(summary, phase_calls=0, split=0, haplotypes=0)
    site_pm, r2_pm = permille(args.min_site_share), permille(args.min_r2)
    single_pm, hap_pm = permille(args.single_share), permille(args.min_hap_share)
    plan = specimine.plan_calls([(consensus.specimen_cost(r.path, r, args.min_cluster_size), []) for r in results], budget)
    for call in plan:
        groups, owner = [], []
        for i in sorted(call):
            for ph in phased[i]:
                groups.append([results[i].records[x].seq for x in results[i].clusters[ph.pc.rank - 1]])
                owner.append(ph)
        if not groups:
            continue
        # the members of every cluster back to back, then every cluster's final consensus: the draft of its job
        reads = [r.encode("latin-1") for g in groups for r in g] + [ph.pc.seq.encode("latin-1") for ph in owner]
        ks = [specimine.max_distance(len(r), args.min_identity) for r in reads]
        jobs, at = [], 0
        for g, group in enumerate(groups):
            jobs.append((len(reads) - len(groups) + g, at, len(group)))
            at += len(group)
        summary["phase_calls"] += 1
        hap_groups, hap_drafts, hap_owner = [], [], []
        for ph, group, jp in zip(owner, groups, phase_fn(reads, ks, jobs, site_pm, args.min_cluster_size, args.max_sites,
                                                         kernel_ms)):
            ph.aligned, ph.sites, ph.n_qualified = jp.aligned, list(jp.sites), jp.n_qualified
            ph.partners, ph.accepted = accept_sites(ph.sites, jp.link, jp.aligned, args.min_cluster_size, r2_pm, single_pm)
            which = [s for s, ok in enumerate(ph.accepted) if ok]
            found, unassigned = haplotypes(member_calls(jp.planes, which, len(group)), jp.aligned, args.min_cluster_size,
                                           hap_pm)
            if len(found) < 2:
                continue
            ph.unassigned = len(unassigned)
            for h, (sig, members) in enumerate(found, 1):
                hap = Haplotype(h, sig, members)
                ph.haps.append(hap)
                hap_groups.append([group[x] for x in members])
                hap_drafts.append(ph.pc.seq)
                hap_owner.append(hap)
            summary["split"] += 1
            summary["haplotypes"] += len(found)
        if hap_groups:
            done, n_calls = consensus.polish(hap_groups, args.min_identity, args.rounds, args.min_cluster_size, votes_fn,
                                             kernel_ms, drafts=hap_drafts)
            summary["vote_calls"] += n_calls
            for hap, (seq, aligned, nrounds, stop) in zip(hap_owner, done):
                hap.seq, hap.aligned, hap.rounds, hap.stop = seq, aligned, nrounds, stop
    return results, polished, phased, summary


# ------------------------------------------------------------------------------------------------ outputs
COLUMNS = ("specimen", "status", "sampled", "cluster", "haplotype", "size", "share", "sites", "aligned", "rounds", "stop",
           "length", "name")
SITE_COLUMNS = ("specimen", "cluster", "pos", "kind", "major", "minor", "n_major", "n_minor", "partners", "accepted", "clipped")


def allele(site: Site, code: int) -> str:
    return ("absent", "present")[code] if site.kind else ALLELES[code]


def signature_text(ph: Phased, hap: Haplotype) -> str:
    """The haplotype's allele at every accepted site: <pos><A|C|G|T|-> for a base, <pos>i+ / <pos>i- for an insertion
    present / absent before pos; joined by commas."""
    which = [s for s, ok in enumerate(ph.accepted) if ok]
    out = []
    for s, bit in zip(which, hap.signature):
        site = ph.sites[s]
        code = site.minor if bit else site.major
        out.append(f"{site.pos}{('i-', 'i+')[code] if site.kind else ALLELES[code]}")
    return ",".join(out)


def cluster_docs(res: clusters.SpecimenResult, phs: Sequence[Phased]) -> List[Dict]:
    """consensus.cluster_docs with every split cluster replaced by its haplotypes."""
    out = []
    for doc, ph in zip(consensus.cluster_docs(res, [ph.pc for ph in phs]), phs):
        if not ph.haps:
            out.append(doc)
            continue
        for hap in ph.haps:
            out.append({"name": f"{doc['name']}_h{hap.index}", "rank": doc["rank"], "haplotype": hap.index,
                        "parent": doc["name"], "size": len(hap.members),
                        "share": round(len(hap.members) / len(res.sampled), 4), "sites": signature_text(ph, hap),
                        "aligned": hap.aligned, "rounds": hap.rounds, "stop": hap.stop, "length": len(hap.seq),
                        "consensus": hap.seq})
    return out


def fasta_text(results, phased) -> str:
    """A single cluster's record is specimux-consensus' own; a split cluster has one record per haplotype."""
    out = []
    for res, phs in zip(results, phased):
        for ph in phs:
            if not ph.haps:
                out.append(consensus.fasta_text([res], [[ph.pc]]))
                continue
            for d in cluster_docs(res, [ph]):
                out.append(f">{d['name']} size={d['size']} share={d['share']:.4f} sites={d['sites']} aligned={d['aligned']} "
                           f"rounds={d['rounds']}\n{d['consensus']}\n")
    return "".join(out)


def tsv_text(results, phased) -> str:
    lines = ["\t".join(COLUMNS)]
    for res, phs in zip(results, phased):
        for d in cluster_docs(res, phs):
            lines.append("\t".join(str(x) for x in (res.path, res.status, len(res.sampled), d["rank"], d.get("haplotype", "-"),
                                                    d["size"], f"{d['share']:.4f}", d.get("sites", "-"), d["aligned"],
                                                    d["rounds"], d["stop"], d["length"], d["name"])))
    return "\n".join(lines) + "\n"


def sites_text(results, phased) -> str:
    lines = ["\t".join(SITE_COLUMNS)]
    for res, phs in zip(results, phased):
        for ph in phs:
            clipped = "clipped" if ph.n_qualified > len(ph.sites) else "-"
            for s, site in enumerate(ph.sites):
                lines.append("\t".join(str(x) for x in (
                    res.path, ph.pc.rank, site.pos, ("base", "insertion")[site.kind], allele(site, site.major),
                    allele(site, site.minor), site.n_major, site.n_minor,
                    ",".join(str(ph.sites[t].pos) + ("i" if ph.sites[t].kind else "") for t in ph.partners[s]) or "-",
                    ("no", "yes")[ph.accepted[s]], clipped)))
    return "\n".join(lines) + "\n"


def json_text(results, phased, summary: Dict) -> str:
    return json.dumps({"summary": summary,
                       "specimens": [{"specimen": res.path, "reads": len(res.records), "sampled": len(res.sampled),
                                      "status": res.status, "clusters": cluster_docs(res, phs)}
                                     for res, phs in zip(results, phased)]}, indent=1) + "\n"


def summary_line(summary: Dict) -> str:
    return (f"Split {summary['split']} of {summary['polished']} cluster(s) of {summary['read']} specimen(s) into "
            f"{summary['haplotypes']} haplotype(s) in {summary['phase_calls']} phase call(s)")


def run(args, adjacency_fn: Callable = clusters.adjacency, votes_fn: Callable = consensus.votes, phase_fn: Callable = phase,
        kernel_ms: Optional[list] = None) -> int:
    """Everything main() does after parsing; returns the exit status (1 only if no file could be read)."""
    if not 1 <= args.max_sites <= MAX_SITES:
        logging.error(f"--max-sites must be in 1..{MAX_SITES}")
        return 2
    paths = [args.fastq] if args.fastq else specimine.discover_specimens(args.run_dir, args.level)
    results, _polished, phased, summary = variants_files(paths, args, adjacency_fn, votes_fn, phase_fn, kernel_ms)
    if summary["read"] == 0:
        logging.error("No specimen file could be read")
        return 1
    for res, phs in zip(results, phased):
        for ph in phs:
            if ph.n_qualified > len(ph.sites):
                logging.warning(f"{res.path}: cluster {ph.pc.rank}: {ph.n_qualified} sites qualified, the first "
                                f"{len(ph.sites)} were kept (--max-sites)")
    logging.info(summary_line(summary))
    specimine.write_texts(((args.fasta, lambda: fasta_text(results, phased)), (args.report, lambda: tsv_text(results, phased)),
                           (args.json, lambda: json_text(results, phased, summary)),
                           (args.sites, lambda: sites_text(results, phased))))
    return 0


def main(argv=None):
    specimine.tool_main(build_parser, run, argv)


if __name__ == "__main__":
    main()
