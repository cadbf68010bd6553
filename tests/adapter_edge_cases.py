"""Case builders shared by the adapter-finder edge tests (CPU: test_adapter_oracle_host.py, GPU: test_gpu_adapter_edges.py).
A plain module, no fixtures: everything is a pure, seeded function of its arguments, so both files see the same inputs.

A group is a list of Batch objects: one adapter table (Handle.set_splints) and the reads scanned against it, every read
against every adapter on both strands.  A batch also carries *claims*: (read, adapter, strand, kind, detail) tuples that say
which pair was built for which mechanism of k_adapter.  The host tests assert every claim on the oracle's output (so a group
cannot silently stop reaching the code it is for); the comparison kernel == oracle runs over all pairs of a batch, claimed or not.

Columns are DP columns: column j (1-based) is adapter base j - 1 of the strand's column sequence; k_adapter computes columns
64 c + 1 .. 64 c + 64 in one pass of the wave, so the seams lie between columns 64 | 65, 128 | 129, ...

Groups and what they are for:
  seams()   adapter lengths at the chunk seams and at the table limit, exact / substituted / short reads: carry_old, carry_h
  hgaps()   one horizontal (target-side) gap across a seam, and one across a whole chunk: carry_f, the fx flag, tBaseInsert
  vgaps()   one vertical (query-side) gap next to a seam: Erow, the ex flag, qBaseInsert
  ties()    equal maxima in other rows, in other chunks of one row, everywhere: the first-maximum rule
  queue(n)  many short, mixed items: a wave takes several items one after the other (LDS rows, direction bytes reused)
"""
import numpy as np

MATCH, MISMATCH, GAP_OPEN, GAP_EXT = 2, -4, 4, 2          # match 2, mismatch -4, gap 4 + 2k
SPLINT_MAX = 512                                          # rows of the splint table hold at most 512 bases
FIELDS = ("score", "qStart", "qEnd", "tStart", "tEnd", "matches", "misMatches", "qBaseInsert", "tBaseInsert", "qNumInsert",
          "tNumInsert", "qSize")
_COMP = str.maketrans("ACGTNacgtn", "TGCANtgcan")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def rand_seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def other_base(c, step=1):
    return "ACGT"[("ACGT".index(c) + step) % 4]


def noisy(rng, s, err):
    """s with substitutions (40 %), insertions (25 %) and deletions (35 %) at a total rate of err per base"""
    out = []
    for c in s:
        u = rng.random()
        if u < err * 0.35:
            continue
        if u < err * 0.75:
            c = other_base(c, int(rng.integers(1, 4)))
        out.append(c)
        if rng.random() < err * 0.25:
            out.append("ACGT"[int(rng.integers(0, 4))])
    return "".join(out)


class Batch:
    def __init__(self, name, purpose, adapters):
        self.name, self.purpose, self.adapters = name, purpose, list(adapters)
        self.reads = []
        self.claims = []                # (read index, adapter index, strand, kind, detail)

    def add(self, read, *claims):
        """append a read; claims = (adapter index, strand, kind, detail) of the pairs this read was built for"""
        self.reads.append(read)
        for a, s, kind, detail in claims:
            self.claims.append((len(self.reads) - 1, a, s, kind, detail))
        return len(self.reads) - 1

    def n_items(self):
        return len(self.reads) * len(self.adapters) * 2

    def scratch_bytes(self, grid_cap):
        """the direction bytes c3_scan_adapters allocates for this batch on a device that runs at most grid_cap waves"""
        dcap = (max(map(len, self.reads)) + 1) * (max(map(len, self.adapters)) + 1) + 64
        return dcap * min(self.n_items(), grid_cap)

    def __repr__(self):
        return "Batch(%s: %d adapters x %d reads)" % (self.name, len(self.adapters), len(self.reads))


# ---- field consistency (both test files) -----------------------------------------------------------------------------------
def check_fields(row, L, m, where=None):
    """the twelve fields of one (read, adapter, strand) row agree with one another, whatever alignment they describe"""
    sc, qs, qe, ts, te, ma, mm, qbi, tbi, qni, tni, qsz = (int(v) for v in row)
    ctx = (where, dict(zip(FIELDS, (int(v) for v in row))), L, m)
    assert qsz == L, ctx
    assert sc >= 0, ctx
    if sc == 0:
        assert (qs, qe, ts, te, ma, mm, qbi, tbi, qni, tni) == (0,) * 10, ctx
        return
    assert sc == MATCH * ma + MISMATCH * mm - GAP_OPEN * (qni + tni) - GAP_EXT * (qbi + tbi), ctx
    assert qe - qs == ma + mm + qbi, ctx
    assert te - ts == ma + mm + tbi, ctx
    assert 0 <= qs <= qe <= L and 0 <= ts <= te <= m, ctx
    assert 0 <= qni <= qbi and 0 <= tni <= tbi and ma >= 0 and mm >= 0, ctx
    assert (qni == 0) == (qbi == 0) and (tni == 0) == (tbi == 0), ctx


def check_table(batch, tab):
    """check_fields on every row of a table [reads][adapters][2][12] of one batch"""
    assert tab.shape == (len(batch.reads), len(batch.adapters), 2, 12), (batch, tab.shape)
    for i, rd in enumerate(batch.reads):
        for a, ad in enumerate(batch.adapters):
            for s in (0, 1):
                check_fields(tab[i, a, s], len(rd), len(ad), (batch.name, i, a, s))


_oracle_tables = {}


def oracle_table(batch):
    """the oracle's table [reads][adapters][2][12] of a batch: computed once, shared by the tests that need it, read-only"""
    from oracle import oracle_py as O
    if batch.name not in _oracle_tables:
        P = O.default_params()
        t = np.zeros((len(batch.reads), len(batch.adapters), 2, 12), dtype=np.int32)
        for i, rd in enumerate(batch.reads):
            for a, ad in enumerate(batch.adapters):
                for s in (0, 1):
                    t[i, a, s] = O.adapter_align(rd, ad, bool(s), params=P)
        t.setflags(write=False)
        _oracle_tables[batch.name] = t
    return _oracle_tables[batch.name]


# ---- seams -----------------------------------------------------------------------------------------------------------------
SEAM_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 511, 512)
# adapter sets: the direction scratch grows with (longest read + 1) * (longest adapter + 1), so 511 / 512 stay among
# themselves (with one short adapter: three rows, for the subset runs of the order test) and their reads stay short
SEAM_SETS = ((1, 2, 63, 64, 65), (127, 128, 129), (191, 192, 193), (33, 511, 512))
SEAM_COLUMNS = (64, 65, 128, 129)
SHORT_READS = (1, 2, 63, 64, 65)


def seams():
    assert set(SEAM_LENGTHS) <= {m for s in SEAM_SETS for m in s}
    out = []
    for k, lens in enumerate(SEAM_SETS):
        rng = np.random.default_rng([49, 1, k])
        ads = [rand_seq(rng, m) for m in lens]
        b = Batch("seams_%s" % "_".join(map(str, lens)),
                  "adapter lengths %s: columns on either side of a 64-column seam, the last chunk full / one short / one over" % (lens,), ads)
        for a, ad in enumerate(ads):
            m = len(ad)
            b.add(ad, (a, 0, "exact", None))
            b.add(revcomp(ad), (a, 1, "exact", None))
            for col in SEAM_COLUMNS:
                if col > m:
                    continue
                sub = ad[:col - 1] + other_base(ad[col - 1]) + ad[col:]
                # one mismatch inside the alignment needs both flanks to be worth more than it costs (2 * flank > 4); at the
                # last columns the alignment ends before the substitution instead: still a read, no claim
                inside = min(col - 1, m - col) >= 3
                b.add(sub, *([(a, 0, "sub", col)] if inside else []))
                rsub = revcomp(ad)
                rsub = rsub[:col - 1] + other_base(rsub[col - 1]) + rsub[col:]
                b.add(rsub, *([(a, 1, "sub", col)] if inside else []))
            if m >= 8:                                  # a read shorter than the adapter that is a substring of it, across a seam if there is one
                lo = max(0, min(m - 5, 64) - m // 3)
                hi = min(m - 1, lo + max(4, 2 * m // 3))
                b.add(ad[lo:hi], (a, 0, "substring", (lo, hi)))
                b.add(revcomp(ad[lo:hi]), (a, 1, "substring", (lo, hi)))
        longest = ads[-1]
        for L in SHORT_READS:
            b.add(rand_seq(rng, L))
            if L < len(longest):
                b.add(longest[-L:], (len(ads) - 1, 0, "substring", (len(longest) - L, len(longest))))
        b.add("", (0, 0, "empty", None), (0, 1, "empty", None))         # c3_batch_upload takes a read of length 0
        out.append(b)
    return out


# ---- horizontal gaps -------------------------------------------------------------------------------------------------------
HGAP_KS = (1, 2, 5, 20)


def _straddle(seam, k):
    """first of k columns (1-based) placed around the seam between columns seam | seam + 1"""
    return seam + 1 - (k + 1) // 2


def hgap_placements(m):
    """[(first removed column, k)] for an adapter of m bases"""
    out = [(_straddle(seam, k), k) for seam in (64, 128) for k in HGAP_KS]
    if m == 512:
        out.append((121, 80))           # adapter bases 120 .. 199: all of chunk 129 .. 192 lies inside the gap, two seams crossed
    return out


def hgaps():
    rng = np.random.default_rng([49, 2])
    ads = [rand_seq(rng, 512), rand_seq(rng, 200)]
    b = Batch("hgaps", "the read lacks k adapter bases: one horizontal gap across a seam (carry_f, carry_h, fx) or across a whole chunk", ads)
    for a, ad in enumerate(ads):
        m = len(ad)
        for strand in (0, 1):
            cols = revcomp(ad) if strand else ad               # the column sequence of this strand
            for first, k in hgap_placements(m):
                left, right = first - 1, m - (first - 1 + k)
                assert 2 * min(left, right) > GAP_OPEN + GAP_EXT * k, (m, first, k)
                rd = cols[:first - 1] + cols[first - 1 + k:]
                b.add(rd, (a, strand, "hgap", k))
                # the same read reverse-complemented aligns to the other strand; there the gap lies at the mirrored columns
                b.add(revcomp(rd), (a, 1 - strand, "hgap", k))
    return [b]


# ---- vertical gaps ---------------------------------------------------------------------------------------------------------
VGAP_AFTER = (63, 64, 100)
VGAP_KS = (1, 2, 7, 40)


def vgaps():
    rng = np.random.default_rng([49, 3])
    ads = [rand_seq(rng, 200), rand_seq(rng, 193)]
    b = Batch("vgaps", "the read has k extra bases after adapter column 63 / 64 / 100: one vertical gap (Erow, ex) at a seam and inside a chunk", ads)
    for a, ad in enumerate(ads):
        m = len(ad)
        for strand in (0, 1):
            cols = revcomp(ad) if strand else ad
            for after in VGAP_AFTER:
                for k in VGAP_KS:
                    assert 2 * min(after, m - after) > GAP_OPEN + GAP_EXT * k, (m, after, k)
                    # the inserted run neither starts nor ends with a neighbour's base: the gap cannot trade a base with a flank
                    ins = rand_seq(rng, k)
                    while ins[0] in (cols[after - 1], cols[after]) or ins[-1] in (cols[after - 1], cols[after]):
                        ins = rand_seq(rng, k)
                    rd = cols[:after] + ins + cols[after:]
                    b.add(rd, (a, strand, "vgap", k))
                    b.add(revcomp(rd), (a, 1 - strand, "vgap", k))
    return [b]


# ---- ties ------------------------------------------------------------------------------------------------------------------
def _flank(rng, n, not_first=None, not_last=None):
    """n random bases; not_first: the flank's first bases differ from these, one by one; not_last: its last base differs"""
    s = list(rand_seq(rng, n))
    for k, c in enumerate(not_first or ""):
        if s[k] == c:
            s[k] = other_base(s[k])
    if not_last is not None and s[-1] == not_last:
        s[-1] = other_base(s[-1])
    return "".join(s)


def ties():
    rng = np.random.default_rng([49, 4])
    a40, x = rand_seq(rng, 40), rand_seq(rng, 70)
    ads = [a40, x + x, "A" * 65, "A" * 129, "AC" * 40, "CA" * 33, "A" * 64, "A" * 130]
    A40, XX, A65, A129, AC40, CA33, A64, A130 = range(8)
    b = Batch("ties", "equal maxima: two rows, two chunks of one row, whole plateaus; a read without any positive cell", ads)
    # two exact copies 200 bases apart: the same maximum in two rows, the earlier row wins
    pre = _flank(rng, 30)
    b.add(pre + a40 + _flank(rng, 200) + a40 + _flank(rng, 30), (A40, 0, "tie", None), (A40, 0, "qEnd", len(pre) + 40))
    rd = _flank(rng, 30) + revcomp(a40) + _flank(rng, 200) + revcomp(a40) + _flank(rng, 30)
    b.add(rd, (A40, 1, "tie", None), (A40, 1, "qEnd", 70))
    # X once against X + X: 2 |X| at columns 70 and 140 of one row (chunks 1 and 2).  The flanks must not extend either copy: the base
    # before X differs from X's last one, the four bases after X from X's first four (no way back to 2 |X| in a later row)
    pre = _flank(rng, 25, not_last=x[-1])
    post = _flank(rng, 25, not_first=x[:4])
    b.add(pre + x + post, (XX, 0, "tie_xx", len(pre) + 70))
    rx = revcomp(x)
    pre = _flank(rng, 25, not_last=rx[-1])
    post = _flank(rng, 25, not_first=rx[:4])
    b.add(pre + rx + post, (XX, 1, "tie_xx", len(pre) + 70))
    # homopolymers: every cell of the last full row / column holds the maximum
    b.add("A" * 64, (A65, 0, "tie", None), (A129, 0, "tie", None), (A130, 0, "tie", None))
    b.add("A" * 130, (A129, 0, "tie", None), (A65, 0, "tie", None), (A64, 0, "tie", None))
    b.add("A" * 65, (A64, 0, "tie", None))
    b.add("A" * 129, (A130, 0, "tie", None))
    b.add("T" * 64, (A65, 1, "tie", None), (A129, 1, "tie", None))
    b.add("T" * 130, (A129, 1, "tie", None), (A65, 1, "tie", None))
    # period 2: a maximum every second row
    b.add("AC" * 100, (AC40, 0, "tie", None), (CA33, 0, "tie", None))
    b.add("GT" * 100, (AC40, 1, "tie", None), (CA33, 1, "tie", None))
    # N (coded as A) and lower case
    b.add("N" * 25 + a40 + "nnnn")
    b.add("N" * 25 + a40.lower() + x.lower()[:30] + "nnnn", (A40, 0, "qEnd", 65))
    b.add("N" * 70 + "n" * 70, (A65, 0, "tie", None))
    # no positive cell at all: G matches neither A (strand 0) nor T (strand 1)
    b.add("G" * 50, *[(a, s, "zero", None) for a in (A65, A129, A64, A130) for s in (0, 1)])
    b.add("g", *[(a, s, "zero", None) for a in (A65, A129) for s in (0, 1)])
    return [b]


# ---- queue -----------------------------------------------------------------------------------------------------------------
QUEUE_ADAPTER_LENGTHS = (20, 64, 65, 200)


def queue(exceed):
    """a batch of at least 3 * exceed items: short reads (20 .. 200 bases) against four adapters, ordered so that the length
    jumps from one read to the next (successive items of a wave differ in both L and m: the direction bytes of the item before
    lie under another row stride)"""
    rng = np.random.default_rng([49, 5])
    ads = [rand_seq(rng, m) for m in QUEUE_ADAPTER_LENGTHS]
    n_reads = -(-3 * exceed // (2 * len(ads)))
    borrowed = [r for g in (seams(), hgaps(), vgaps(), ties()) for bt in g for r in bt.reads if 20 <= len(r) <= 200]
    pool = []
    for i in range(n_reads):
        kind = i % 3
        if kind == 0:                   # a noisy adapter on either strand between random flanks
            ad = ads[int(rng.integers(0, 4))]
            core = noisy(rng, revcomp(ad) if rng.integers(0, 2) else ad, float(rng.choice([0.0, 0.05, 0.15])))
            core = core[:int(rng.integers(15, 201))]
            room = 200 - len(core)
            lf = int(rng.integers(0, room + 1)) if room else 0
            rd = rand_seq(rng, lf) + core + rand_seq(rng, int(rng.integers(0, room - lf + 1)))
            rd = rd if len(rd) >= 20 else rd + rand_seq(rng, 20 - len(rd))
        elif kind == 1:
            rd = rand_seq(rng, int(rng.integers(20, 201)))
        else:
            rd = borrowed[int(rng.integers(0, len(borrowed)))]
        assert 20 <= len(rd) <= 200
        pool.append(rd)
    pool.sort(key=len)
    reads = []
    lo, hi = 0, len(pool) - 1
    while lo <= hi:                      # shortest, longest, second shortest, ...
        reads.append(pool[lo]); lo += 1
        if lo <= hi:
            reads.append(pool[hi]); hi -= 1
    b = Batch("queue_%d" % exceed, "more items than waves: every wave runs the persistent loop several times", ads)
    for r in reads:
        b.add(r)
    assert b.n_items() >= 3 * exceed
    return b


# ---- random small pairs (host tests) ---------------------------------------------------------------------------------------
def random_pairs(n, seed=6):
    """[(read, adapter)] with lengths 1 .. 150: unrelated, or the read holds a noisy copy of the adapter or of its reverse
    complement"""
    rng = np.random.default_rng([49, seed])
    out = []
    for i in range(n):
        ad = rand_seq(rng, int(rng.integers(1, 151)))
        kind = i % 4
        if kind == 0:
            rd = rand_seq(rng, int(rng.integers(1, 151)))
        else:
            core = noisy(rng, revcomp(ad) if kind == 3 else ad, float(rng.choice([0.02, 0.1, 0.25])))
            rd = (rand_seq(rng, int(rng.integers(0, 30))) + core + rand_seq(rng, int(rng.integers(0, 30))))[:150]
            if kind == 2:                # small alphabet: many equal maxima and gap placements
                rd = rd.replace("G", "A").replace("T", "C")
                ad = ad.replace("G", "A").replace("T", "C")
        out.append((rd or "A", ad))
    return out


def groups():
    """{group name: [Batch]} of the designed groups (queue(n) depends on the device and is built by its user)"""
    return {"seams": seams(), "hgaps": hgaps(), "vgaps": vgaps(), "ties": ties()}
