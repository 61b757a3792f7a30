"""The allele-specific methylation report (include/epihip.h, epi_batch_asm_report_dev) restated as plain loops: one loop per
rule of the definitions, nothing vectorised, no GPU.  Also the helper that packs templates with a base per position
(helpers.templates_from_xm has one base for all), and the fuzz batches of tests/test_gpu_fuzz_asm.py.  Test infrastructure only."""
import bisect

import numpy as np

NA_INT = -2 ** 31
NT16 = {"A": 1, "C": 2, "G": 4, "T": 8, "N": 15, "-": 15}          # '-': the 0xF? filler between mates
NT16_INT = (4, 0, 1, 4, 2, 4, 4, 4, 3, 4, 4, 4, 4, 4, 4, 4)          # HTSlib's seq_nt16_int
METH_CODES = (2, 5, 6, 7)
UNMETH_CODES = (10, 13, 14, 15)
PAIR_INT = ("snv", "rname", "snv_pos", "strand", "pos", "context", "meth_ref", "unmeth_ref", "meth_alt", "unmeth_alt")
SNV_INT = ("rname", "pos", "reads_ref", "reads_alt", "reads_other", "npairs", "meth_ref", "unmeth_ref", "meth_alt", "unmeth_alt")
DOUBLES = ("beta_ref", "beta_alt", "delta_beta", "p")
PAIR_COLUMNS = PAIR_INT + DOUBLES
SNV_COLUMNS = SNV_INT + DOUBLES
CELLS = ("meth_ref", "unmeth_ref", "meth_alt", "unmeth_alt")
# R/internal.R:642-666 by hand, as (REF '+', ALT '+', REF '-', ALT '-') base sets: not read from the package
ALLELES = {("A", "C"): ("A", "CT", "A", "C"), ("A", "T"): ("A", "T", "A", "T"), ("A", "G"): ("A", "G", "", ""),
           ("C", "A"): ("CT", "A", "C", "A"), ("C", "T"): ("", "", "C", "T"), ("C", "G"): ("CT", "G", "C", "AG"),
           ("T", "A"): ("T", "A", "T", "A"), ("T", "C"): ("", "", "T", "C"), ("T", "G"): ("T", "G", "T", "AG"),
           ("G", "A"): ("G", "A", "", ""), ("G", "C"): ("G", "CT", "AG", "C"), ("G", "T"): ("G", "T", "AG", "T")}


def ctx_to_idx(ch):
    return ((ord(ch) + 2) >> 2) & 15


def mask_of(ref, alt):
    """site_alleles of one (REF, ALT) pair, from the hand-written table above; 0 for a pair that is not in it"""
    sets = ALLELES.get((ref, alt), ("", "", "", ""))
    mask = 0
    for k, bases in enumerate(sets):
        for base in bases:
            mask |= (1 << "ACGT".index(base)) << (4 * k)
    return mask


def templates(xms, seqs, starts, strands, rnames=None):
    """Packed templates from XM strings and base strings of the same lengths (A, C, G, T, N, '-' for the filler between
    mates): byte = (nt16 << 4) | ctx_to_idx(XM letter); rows sorted by (rname, start), stable."""
    n = len(xms)
    rnames = [1] * n if rnames is None else list(rnames)
    order = sorted(range(n), key=lambda i: (rnames[i], starts[i], i))
    rows = []
    for i in order:
        assert len(xms[i]) == len(seqs[i]), i
        rows.append(np.asarray([(NT16[b] << 4) | ctx_to_idx(c) for c, b in zip(xms[i], seqs[i])], np.uint8))
    off = np.zeros(n + 1, np.int64)
    for k, r in enumerate(rows):
        off[k + 1] = off[k] + r.size
    return {"xm": np.concatenate(rows).astype(np.uint8) if rows and off[-1] else np.zeros(0, np.uint8), "off": off,
            "rname": np.asarray([rnames[i] for i in order], np.int32),
            "strand": np.asarray([strands[i] for i in order], np.int32),
            "start": np.asarray([starts[i] for i in order], np.int32)}


def ratio(a, b):
    return np.float64(a) / np.float64(b) if b else np.float64("nan")


def restate(t, site_chr, site_pos, site_alleles, ctx, max_distance=0, min_coverage=1, max_oo=0.1, fisher=None, events=None):
    """-> (pairs, snvs): dicts of numpy columns (PAIR_COLUMNS, SNV_COLUMNS; without p unless `fisher`, a function of four
    integer arrays, is given).  The sites are taken in the order given (any order); `snv` indexes it.  events: a list that
    receives the number of events of every site, reported or not."""
    xm, off, rname, strand, start = t["xm"], t["off"], t["rname"], t["strand"], t["start"]
    nsite = len(site_chr)
    ctx_codes = {ctx_to_idx(c) for c in ctx}
    by_chr = {}                                              # chr -> sorted [(pos, site)]
    for s in range(nsite):
        if int(site_chr[s]) != NA_INT:
            by_chr.setdefault(int(site_chr[s]), []).append((int(site_pos[s]), s))
    for v in by_chr.values():
        v.sort()
    reads = np.zeros((nsite, 3), np.int64)
    cells = {}                                               # (site, q, strand, context code) -> four cells
    for x in range(len(start)):
        length = int(off[x + 1] - off[x])
        if strand[x] not in (1, 2) or length <= 0 or int(rname[x]) == NA_INT:
            continue
        codes = [int(b) & 15 for b in xm[off[x]:off[x + 1]]]
        # the read rule: out-of-context methylated over out-of-context calls
        o_m = o_u = 0
        for c in codes:
            if c not in ctx_codes:
                o_m += c in METH_CODES
                o_u += c in UNMETH_CODES
        if o_m + o_u and np.float64(o_m) / np.float64(o_m + o_u) > max_oo:
            continue
        calls = [(i, c) for i, c in enumerate(codes) if c in ctx_codes]
        first, last = int(start[x]), int(start[x]) + length - 1
        cand = by_chr.get(int(rname[x]), [])
        for k in range(bisect.bisect_left(cand, (first, -1)), len(cand)):
            p, s = cand[k]
            if p > last:
                break
            # the allele of the row at the site
            base = NT16_INT[int(xm[off[x] + p - first]) >> 4]
            bit = (1 << base) if base < 4 else 0
            mask = int(site_alleles[s]) >> (0 if strand[x] == 1 else 8)
            allele = 0 if mask & 15 & bit else 1 if (mask >> 4) & 15 & bit else None
            reads[s, 2 if allele is None else allele] += 1
            if allele is None:
                continue
            # its events
            for i, c in calls:
                q = first + i
                if q == p or (max_distance > 0 and abs(q - p) > max_distance):
                    continue
                cell = cells.setdefault((s, q, int(strand[x]), c & 7), [0, 0, 0, 0])
                cell[2 * allele + (0 if c < 8 else 1)] += 1
    if events is not None:
        events[:] = [0] * nsite
        for key, c in cells.items():
            events[key[0]] += sum(c)
    mc = max(int(min_coverage), 1)
    rows = []
    for key in sorted(cells):
        c = cells[key]
        if c[0] + c[1] >= mc and c[2] + c[3] >= mc:
            rows.append((key[0], int(site_chr[key[0]]), int(site_pos[key[0]]), key[2], key[1], key[3]) + tuple(c))
    pairs = {k: np.asarray([r[j] for r in rows], np.int32) for j, k in enumerate(PAIR_INT)}
    snv_rows = []
    for s in range(nsite):
        mine = [r for r in rows if r[0] == s] if int(site_chr[s]) != NA_INT else []
        snv_rows.append((int(site_chr[s]), int(site_pos[s]), reads[s, 0], reads[s, 1], reads[s, 2], len(mine)) +
                        tuple(sum(r[6 + v] for r in mine) for v in range(4)))
    snvs = {k: np.asarray([r[j] for r in snv_rows], np.int32) for j, k in enumerate(SNV_INT)}
    for tab in (pairs, snvs):
        n = len(tab["meth_ref"])
        tab["beta_ref"] = np.asarray([ratio(tab["meth_ref"][i], int(tab["meth_ref"][i]) + int(tab["unmeth_ref"][i])) for i in range(n)], np.float64)
        tab["beta_alt"] = np.asarray([ratio(tab["meth_alt"][i], int(tab["meth_alt"][i]) + int(tab["unmeth_alt"][i])) for i in range(n)], np.float64)
        tab["delta_beta"] = tab["beta_alt"] - tab["beta_ref"]
        if fisher is not None:
            tab["p"] = np.asarray(fisher(*[tab[k] for k in CELLS]), np.float64).reshape(-1) if n else np.zeros(0, np.float64)
    if fisher is not None:
        snvs["p"] = np.where(np.asarray(site_chr, np.int64) == NA_INT, np.nan, snvs["p"])
    return pairs, snvs


def same(got, want, label="", skip=("p",)):
    """Integer columns equal, beta_ref, beta_alt and delta_beta bit for bit; p is compared by the caller"""
    for k, w in want.items():
        if k in skip:
            continue
        g = np.asarray(got[k])
        assert g.shape == w.shape, (label, k, g.shape, w.shape)
        if w.dtype == np.float64:
            assert g.dtype == np.float64 and np.array_equal(g.view(np.uint64), w.view(np.uint64)), (label, k)
        else:
            assert g.dtype == np.int32 and np.array_equal(g, w), (label, k, np.flatnonzero(g != w)[:5])


# ---- fuzz batches -------------------------------------------------------------------------------------------------------------

REF_ALT = sorted(ALLELES)
FUZZ_SEEDS = tuple(range(40))


def fuzz_batch(seed):
    """A fixed-seed batch of at most 2000 rows on two sequences: ragged lengths, both strands, a mate gap of filler bytes in
    some rows, a strand-0 row, bases at the SNVs drawn from REF, ALT and the rest, and SNVs of all twelve REF / ALT pairs
    (three per batch, rotating with the seed, and nine more at random) -> (t, (site_chr, site_pos, site_alleles), (ref, alt),
    args), args the keyword arguments of restate."""
    rng = np.random.default_rng(7000 + seed)
    nrow = int(rng.integers(300, 2001))
    span = int(rng.integers(400, 1500))
    nseq = 2
    starts = np.sort(rng.integers(1, span, nrow))
    rnames = np.sort(rng.integers(1, nseq + 1, nrow))
    lens = rng.integers(1, 181, nrow)
    strands = rng.integers(1, 3, nrow)
    strands[rng.integers(0, nrow)] = 0
    pairs_ = [REF_ALT[(3 * seed + k) % 12] for k in range(3)] + [REF_ALT[int(k)] for k in rng.integers(0, 12, 9)]
    chr_ = rng.integers(1, nseq + 1, len(pairs_))
    pos = rng.integers(20, span + 100, len(pairs_))
    pos[1] = pos[0]                                          # two ALTs at one position
    chr_[1] = chr_[0]
    order = np.lexsort((pos, chr_))
    chr_, pos, pairs_ = chr_[order], pos[order], [pairs_[k] for k in order]
    letters = np.frombuffer(b"ZzXxHh.", np.uint8)
    weights = (0.2, 0.2, 0.01, 0.03, 0.01, 0.05, 0.5)        # a few out-of-context calls: the read rule drops some rows
    bases = np.frombuffer(b"ACGT", np.uint8)
    xms, seqs = [], []
    for x in range(nrow):
        n = int(lens[x])
        xm = letters[rng.choice(letters.size, n, p=weights)].copy()
        sq = bases[rng.integers(0, 4, n)].copy()
        if n > 60 and rng.random() < 0.3:                    # the gap between mates
            a = int(rng.integers(20, n - 20))
            b = a + int(rng.integers(1, 20))
            sq[a:b] = ord("-")
            xm[a:b] = ord(".")
        for k in range(len(pairs_)):                         # at an SNV mostly one of its two alleles
            i = int(pos[k]) - int(starts[x])
            if chr_[k] == rnames[x] and 0 <= i < n and sq[i] != ord("-") and rng.random() < 0.85:
                sq[i] = ord(pairs_[k][int(rng.integers(0, 2))])
        xms.append(xm.tobytes().decode())
        seqs.append(sq.tobytes().decode())
    t = templates(xms, seqs, starts.tolist(), strands.tolist(), rnames.tolist())
    masks = np.asarray([mask_of(r, a) for r, a in pairs_], np.int32)
    args = dict(ctx="Zz", max_distance=(0, 1, 50)[seed % 3], min_coverage=(1, 3)[(seed // 3) % 2], max_oo=0.5)
    return t, (chr_.astype(np.int32), pos.astype(np.int32), masks), pairs_, args


# ---- hand cases -----------------------------------------------------------------------------------------------------------------
# One SNV A>T at position 105 of sequence 1 (REF = A, ALT = T on either strand); rows of 11 bases from 100, the SNV at byte 5.

SNV_POS = 105
A_T, A_C = mask_of("A", "T"), mask_of("A", "C")


def hand_row(xm, base, start=100, strand=1, at=5):
    """(xm, seq, start, strand) with `base` at byte `at` and C elsewhere"""
    return xm, "C" * at + base + "C" * (len(xm) - at - 1), start, strand


def hand_templates(rows):
    return templates([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows])


def hand_cases():
    """name -> (templates, (site_chr, site_pos, site_alleles), restate's keyword arguments).  tests/test_asm_host.py has what
    each must give, written by hand."""
    site = (np.asarray([1], np.int32), np.asarray([SNV_POS], np.int32), np.asarray([A_T], np.int32))
    rules = [hand_row("Z....z...Z.", "A"),                   # REF; its call AT the SNV does not count
             hand_row("z....Z...z.", "T"),                   # ALT
             hand_row("Z........Z.", "-"),                   # the filler between mates at the SNV: no allele
             hand_row("Z........Z.", "A", strand=0),         # no strand: not a row of the report
             hand_row("Z....H...Z.", "A"),                   # 1 of 1 out-of-context calls methylated: dropped
             hand_row("Z.z", "T", start=103, at=2, strand=2),    # ALT on '-': a group of its own, without a REF call
             hand_row("Z........Z.", "G")]                   # a third base
    cases = {"rules": (hand_templates(rules), site, dict(ctx="Zz"))}
    dist = [hand_row("ZZ.......ZZ", "A"), hand_row("zz.......zz", "T")]
    cases["distance"] = (hand_templates(dist), site, dict(ctx="Zz", max_distance=4))
    two = (np.asarray([1, 1], np.int32), np.asarray([SNV_POS, SNV_POS], np.int32), np.asarray([A_T, A_C], np.int32))
    cases["two_alts"] = (hand_templates(rules), two, dict(ctx="Zz"))
    na = (np.asarray([NA_INT, 1], np.int32), np.asarray([7, SNV_POS], np.int32), np.asarray([A_T, A_T], np.int32))
    cases["na_site"] = (hand_templates(rules), na, dict(ctx="Zz"))
    cov = [hand_row("Z........Z.", "A"), hand_row("z..........", "A"), hand_row("z........z.", "T"), hand_row("Z..........", "T")]
    for mc in (1, 2, 3):
        cases["coverage_%d" % mc] = (hand_templates(cov), site, dict(ctx="Zz", min_coverage=mc))
    return cases
