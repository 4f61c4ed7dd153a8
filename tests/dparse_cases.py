"""Crafted texts for the device read parser (metafast_amd/csrc/mf_dparse.hip), in plain Python: no GPU, nothing of the library's.

A case is a text with its format (1 FASTA, 2 FASTQ), the quality offset the host would sniff from it, what is expected of it and what it is
there to reach.  `expect`: "taken" = the device parser is sure about it (rc 0), "back" = it steps back and the host reader makes the
oracle's reads, "error" = it steps back and the readers refuse the file.  `bit`: the anomaly bit a case is about (0: none).  `at`: a list
of (position, bytes) that tests/test_dparse_cases_cpu.py finds in the text, so that a feature provably stands where its name says.

The kernels give a thread 16 bytes, a workgroup's step 4096 (a tile) and a workgroup 262144 (a chunk): BORDERS x OFFSETS are the
positions at which the byte in front of a feature, the feature or the byte behind it belong to another thread, tile or chunk."""
import numpy as np

from dparse_ref import A_BAD_CHAR, A_BAD_QUAL, A_EMPTY_LINE, A_LENGTHS, A_LONE_CR

TILE, CHUNK = 4096, 262144
BORDERS = (16, TILE, CHUNK, CHUNK + TILE)
OFFSETS = (-2, -1, 0, 1)
ENDS = (1, 15, 16, 17, 4095, 4096, 4097, 262143, 262144, 262145)
ENDINGS = {"nl": b"\n", "crlf": b"\r\n", "cr": b"\r", "base": b""}
REC_COUNTS = (255, 256, 257, 2047, 2048, 2049)
SCAN2_RECORDS = 2_097_153 + 2_048            # k_dp_scan2 walks 1024 blocks of 2048 records at a time: 1026 blocks
BIG = 1 << 20                                # texts above this size: the vectorised reference, one fill byte


class Case:
    def __init__(self, name, make, fmt, qoff=33, expect="taken", bit=0, reach="", at=None, span=None, n_rec=None, size=0):
        self.name, self._make, self.fmt, self.qoff, self.expect, self.bit, self.reach = name, make, fmt, qoff, expect, bit, reach
        self.at, self.span, self.n_rec, self.size = at or [], span, n_rec, size
        self._text = None
        self.line_at = None
        self.border_at = None                 # the sweep's cases: P

    @property
    def big(self):
        return self.size > BIG

    @property
    def text(self):
        if self.big:                          # (16 MB each: made when asked for, kept by nobody)
            return self._make()
        if self._text is None:
            self._text = self._make()
        return self._text

    @property
    def ext(self):
        return ".fa" if self.fmt == 1 else ".fq"


def _rng(*key):
    return np.random.default_rng([0x44504152] + [int(k) & 0xFFFFFFFF for k in key])


def bases(rng, n, alphabet=b"ACGTacgt"):
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), size=n)].tobytes()


# ---------------------------------------------------------------------------------------------
# FASTA: a front of exactly L bytes
# ---------------------------------------------------------------------------------------------
def fa_front(rng, L, open_line, wrap=70):
    """L bytes: a header line of about L / 3 bytes whose text is made of base letters (bytes that must not count), then sequence lines of
    `wrap` bytes.  open_line: it ends inside a sequence line with at least one base on it; else with the '\\n' of a line that is not empty"""
    if L < 4:
        return bases(rng, L) if open_line else (bases(rng, L - 1) + b"\n" if L else b"")
    for H in range(max(3, L // 3), L + 1):
        R = L - H
        last = R % wrap
        if (last >= 1) if open_line else (last != 1):               # (closed: no line of the '\n' alone; R == 0: the header line's own '\n' ends it)
            break
    out = [b">", bases(rng, H - 2, b"ACGTN>;"), b"\n"]
    full, last = divmod(R, wrap)
    for _ in range(full):
        out.append(bases(rng, wrap - 1) + b"\n")
    if last:
        out.append(bases(rng, last) if open_line else bases(rng, last - 1) + b"\n")
    t = b"".join(out)
    assert len(t) == L and (open_line or t.endswith(b"\n")) and (not open_line or not t.endswith(b"\n")), (L, open_line, len(t))
    return t


FA_TAIL = b">tail one\nACGTTGCA\nGGA\n>tail two\nTTTACG\n"

# name -> (the front ends inside a line?, what stands at P, what follows on the line, expect, bit, (offset from P, bytes) to find)
FA_FEATURES = {
    "header":        (False, b">x y\n", b"ACGTAC\n", "taken", 0, (-1, b"\n>")),
    "comment":       (False, b";c\n", b"ACGTAC\n", "taken", 0, (-1, b"\n;")),
    "crlf":          (True, b"\r\n", b"ACG\r\n", "taken", 0, (0, b"\r\n")),
    "N":             (True, b"N", b"ACG\n", "taken", 0, (0, b"N")),
    "n":             (True, b"n", b"ACG\n", "taken", 0, (0, b"n")),
    "iupac":         (True, b"R", b"yAC\n", "taken", 0, (0, b"Ry")),
    "lone_cr":       (True, b"\r", b"ACG\n", "back", A_LONE_CR, (0, b"\rA")),
    "bad_char":      (True, b"J", b"ACG\n", "error", A_BAD_CHAR, (0, b"J")),
    "bad_char_in_N": (True, b"J", b"ACNG\n", "taken", 0, (0, b"JACN")),
    "empty_line":    (False, b"\n", b"ACGT\n", "taken", 0, (-1, b"\n\n")),
}


def fa_feature(name, P):
    open_line, here, rest, expect, bit, (off, what) = FA_FEATURES[name]

    def make():
        rng = _rng(1, P, len(name))
        return fa_front(rng, P, open_line) + here + rest + FA_TAIL
    c = Case("fa-%s-at-%d" % (name, P), make, 1, expect=expect, bit=bit, at=[(P + off, what)], reach="FASTA %s at byte %d" % (name, P), size=P + 64)
    c.border_at = P
    return c


def fa_end(n, ending):
    e = ENDINGS[ending]

    def make():
        return fa_front(_rng(2, n, len(e)), n - len(e), ending != "nl") + e if ending != "nl" else fa_front(_rng(2, n, 0), n, False)
    return Case("fa-end-%d-%s" % (n, ending), make, 1, at=[(n - max(len(e), 1), e)] if e else [], reach="a FASTA text of %d bytes that ends in %r" % (n, e), size=n)


def fa_long_seq(L, with_n):
    def make():
        s = bytearray(bases(_rng(3, L), L))
        if with_n:
            s[L - 3] = ord("N")
        return b">a\n" + bytes(s) + b"\n>b\nACGTT\n"
    return Case("fa-line-of-%d-bases%s" % (L, "-N" if with_n else ""), make, 1, span="chunk" if L >= 2 * CHUNK else "tile" if L >= 2 * TILE else None, size=L + 16,
                reach="a sequence line without a line start in a whole %s: the carry of the state from tile to tile%s" % ("chunk" if L >= 2 * CHUNK else "tile", ", chunk state 2 after a chunk that did not end in a header: seq_head counts" if L >= 2 * CHUNK else ""))


def fa_long_header(L):
    def make():
        return b">a\nACGT\n>" + bases(_rng(4, L), L - 2, b"ACGTN") + b"\nACGTTA\n"
    return Case("fa-header-of-%d-bytes" % L, make, 1, span="tile" if L >= 2 * TILE else None, size=L + 16, reach="tiles without a line start inside a header line: base letters that must not count")


def fa_two_long(first):
    """two long records back to back, one of them over a whole chunk: under 700 KB only one chunk can be without a line start, so the two
    orders are two texts"""
    def make():
        rng = _rng(5, len(first))
        if first == "header":
            return b">" + bases(rng, 530000, b"ACGTN") + b"\n" + bases(rng, 150000) + b"\n>t\nAC\n"
        return b">a\n" + bases(rng, 530000) + b"\n>" + bases(rng, 150000, b"ACGTN") + b"\nACGTA\n"
    return Case("fa-long-%s-first" % first, make, 1, span="chunk", size=680100,
                reach="chunk state 2 after a chunk that ended in a %s line: seq_head %s" % (first, "must not count" if first == "header" else "counts"))


# ---------------------------------------------------------------------------------------------
# the flush: e emitted bases in a tile that is header otherwise, behind kept output of every length mod 16
# ---------------------------------------------------------------------------------------------
FLUSH_E = tuple(range(1, 34))


def fa_flush(e):
    def make():
        rng = _rng(6, e)
        out = [b">a\n"]
        size = [3]

        def put(b):
            out.append(b)
            size[0] += len(b)

        def header_to(pos):                                         # a header line whose '\n' stands at pos - 1
            put(b">" + bases(rng, pos - size[0] - 2, b"ACGTN") + b"\n")
        d = (1 - e) % 16 or 16
        for r in range(16):
            t0 = 2 * r + 1
            header_to(t0 * TILE + 2000)
            if r % 2:
                put(b"ACNGT\n>x\n")                                 # a dropped record in front of the e bases, in their tile
            put(bases(rng, e) + b"\n")
            if r % 4 >= 2:
                put(b">y\nNA\n")                                    # ... and one behind them
            header_to((t0 + 1) * TILE + 100)
            put(bases(rng, d) + b"\n")
        return b"".join(out)
    return Case("fa-flush-%d" % e, make, 1, size=33 * TILE, reach="dp_emit_flush: a tile that emits %d bytes, its first one at every place mod 16" % e)


# ---------------------------------------------------------------------------------------------
# record counts, flags
# ---------------------------------------------------------------------------------------------
def fa_records(n_rec, lead):
    def make():
        out = [b"AC\n"] if lead else []
        for i in range(n_rec - 1):
            out.append(b">\n" + (b"" if i % 7 == 3 else b"N\n" if i % 5 == 2 else b"Jn\n" if i % 11 == 6 else (b"A", b"cg", b"TAC")[i % 3] + b"\n"))
        return b"".join(out)
    return Case("fa-%d-records%s" % (n_rec, "-lead" if lead else ""), make, 1, n_rec=n_rec, size=5 * n_rec,
                reach="k_dp_rec_count / k_dp_rec_place with %d records (256 a step, 2048 a block)" % n_rec)


def fa_scan2():
    def make():
        pat = b"".join(b">\n" + x for x in (b"A\n", b"c\n", b"N\n", b"\n\n", b"G\n", b"t\n", b"A\n", b"n\n", b"\r\n", b"R\n", b"C\n", b"A\n", b"T\n", b"N\n", b"G\n", b"A\n"))
        return pat * ((SCAN2_RECORDS - 1) // 16)
    assert (SCAN2_RECORDS - 1) % 16 == 0
    return Case("fa-%d-records" % SCAN2_RECORDS, make, 1, n_rec=SCAN2_RECORDS, size=4 * SCAN2_RECORDS, reach="k_dp_scan2's second step of 1024 blocks: the carry")


def fa_flags(lead, marked, name):
    def make():
        out = [b"ACGT\n" if 0 not in marked else b"ACNT\n"] if lead else []
        for r in range(1, 13):
            out.append(b">r%d\n" % r + (b"AnGT" if r in marked else b"ACGT") + b"\nGG\n")
        return b"".join(out)
    return Case("fa-flags-%s%s" % (name, "-lead" if lead else ""), make, 1, n_rec=13, size=200, reach="rec_flag: four records' flags in a word, N in record(s) %s" % sorted(marked))


# ---------------------------------------------------------------------------------------------
# FASTQ
# ---------------------------------------------------------------------------------------------
def fq_record(rng, m, qoff, extra=0, nl=b"\n", plus=b"+"):
    """a record with m bases, its header `extra` bytes longer than "@r" -> the four lines"""
    q = rng.integers(qoff + 1, min(qoff + 41, 127), size=m).astype(np.uint8)
    q[0] = qoff + 2                                                   # (below 64 for the offset 33: the host sniffs the offset from it)
    return [b"@r" + b"x" * extra + nl, bases(rng, m) + nl, plus + nl, q.tobytes() + nl]


def fq_fill(rng, T, qoff):
    """whole records of T bytes in all -> (text, what is left for the next record's header to take: T < 9 cannot be a record)"""
    if T < 9:
        return b"", T
    out = []
    while T >= 2 * 307:
        out += fq_record(rng, 150, qoff)
        T -= 307
    m = min((T - 7) // 2, 160)
    out += fq_record(rng, m, qoff, extra=T - 7 - 2 * m)
    return b"".join(out), 0


def _fq_with(P, anchor_of, lines_of, qoff, seed):
    """a text whose feature record -- lines_of(rng, extra, m, j) -> four lines -- has the byte anchor_of(lines, m, j) bytes behind its start at P"""
    rng = _rng(7, P, seed)
    m, j = (20, 7) if P >= 64 else (3, 1)                              # (bases of the feature record; the base / quality the feature is)
    T = P - anchor_of(lines_of(_rng(8), 0, m, j), m, j)
    assert T >= 0, (P, T)
    front, extra = fq_fill(rng, T, qoff)
    return front + b"".join(lines_of(rng, extra, m, j)) + b"".join(fq_record(rng, 12, qoff)) + b"".join(fq_record(rng, 5, qoff))


def _line_start(k):
    return lambda lines, m, j: sum(len(x) for x in lines[:k])


def _in_line(k, end=False):
    return lambda lines, m, j: sum(len(x) for x in lines[:k]) + (m if end else j)


def _set(lines, k, j, c):
    b = bytearray(lines[k])
    b[j] = c
    lines[k] = bytes(b)
    return lines


# name -> (anchor, the four lines of the feature record from (rng, extra, m, j), expect, bit, (offset from P, bytes) or the line's number)
FQ_Q = 33
FQ_FEATURES = {
    "line0":      (_line_start(0), lambda g, x, m, j: fq_record(g, m, FQ_Q, x), "taken", 0, 0),
    "line1":      (_line_start(1), lambda g, x, m, j: fq_record(g, m, FQ_Q, x), "taken", 0, 1),
    "line2":      (_line_start(2), lambda g, x, m, j: fq_record(g, m, FQ_Q, x), "taken", 0, 2),
    "line3":      (_line_start(3), lambda g, x, m, j: fq_record(g, m, FQ_Q, x), "taken", 0, 3),
    "plus_is_at": (_line_start(2), lambda g, x, m, j: fq_record(g, m, FQ_Q, x, plus=b"@again"), "taken", 0, (-1, b"\n@again\n")),
    "crlf":       (_in_line(1, True), lambda g, x, m, j: fq_record(g, m, FQ_Q, x, nl=b"\r\n"), "taken", 0, (0, b"\r\n+\r\n")),
    "N":          (_in_line(1), lambda g, x, m, j: _set(fq_record(g, m, FQ_Q, x), 1, j, ord("N")), "taken", 0, (0, b"N")),
    "dot":        (_in_line(1), lambda g, x, m, j: _set(fq_record(g, m, FQ_Q, x), 1, j, ord(".")), "taken", 0, (0, b".")),
    "phred0":     (_in_line(3), lambda g, x, m, j: _set(fq_record(g, m, FQ_Q, x), 3, j, FQ_Q), "taken", 0, (0, bytes([FQ_Q]))),
    "qual_below": (_in_line(3), lambda g, x, m, j: _set(fq_record(g, m, FQ_Q, x), 3, j, FQ_Q - 1), "error", A_BAD_QUAL, (0, bytes([FQ_Q - 1]))),
    "qual_127":   (_in_line(3), lambda g, x, m, j: _set(fq_record(g, m, FQ_Q, x), 3, j, 127), "error", A_BAD_QUAL, (0, b"\x7f")),
    "empty_line": (None, None, "back", A_EMPTY_LINE, (-1, b"\n\n@")),
}


def fq_feature(name, P):
    anchor, lines_of, expect, bit, find = FQ_FEATURES[name]
    if name == "empty_line":                                           # (the empty line stands between two records: the record in front ends at P - 1)
        def make():
            rng = _rng(9, P)
            front, extra = fq_fill(rng, P, FQ_Q)
            assert extra == 0
            return front + b"\n" + b"".join(fq_record(rng, 20, FQ_Q)) + b"".join(fq_record(rng, 5, FQ_Q))
    else:
        def make():
            return _fq_with(P, anchor, lines_of, FQ_Q, len(name))
    c = Case("fq-%s-at-%d" % (name, P), make, 2, qoff=FQ_Q, expect=expect, bit=bit, at=[(P + find[0], find[1])] if isinstance(find, tuple) else [],
             reach="FASTQ %s at byte %d" % (name, P), size=P + 400)
    c.border_at = P
    c.line_at = None if isinstance(find, tuple) else (P, find)         # (P is the first byte of a line with this number mod 4)
    return c


def fq_end(n, ending):
    e = ENDINGS[ending]

    def make():
        rng = _rng(10, n, len(e))
        last = fq_record(rng, 2, FQ_Q)
        last[3] = last[3][:-1] + e
        front, extra = fq_fill(rng, n - sum(len(x) for x in last), FQ_Q)
        last[0] = b"@r" + b"x" * extra + b"\n"
        return front + b"".join(last)
    return Case("fq-end-%d-%s" % (n, ending), make, 2, qoff=FQ_Q, at=[(n - max(len(e), 1), e)] if e else [], reach="a FASTQ text of %d bytes that ends in %r" % (n, e), size=n)


def fq_records(n_rec, qoff):
    def make():
        out = []
        for i in range(n_rec):
            s, q = (b"A", b"cg", b"TAC")[i % 3], bytes([qoff + 5]) * (i % 3 + 1)
            if i % 5 == 2:
                s = b"N" + s[1:]
            if i % 7 == 3:
                q = q[:-1] + bytes([qoff])
            out.append(b"@\n" + s + b"\n+\n" + q + b"\n")
        return b"".join(out)
    return Case("fq-%d-records-phred%d" % (n_rec, qoff), make, 2, qoff=qoff, n_rec=n_rec, size=12 * n_rec, reach="the record kernels with %d FASTQ records, quality offset %d" % (n_rec, qoff))


# ---------------------------------------------------------------------------------------------
# the length limit (16 MB each)
# ---------------------------------------------------------------------------------------------
def fa_limit(over):
    L = (1 << 24) - 1 + over

    def make():
        return b">short\nACGTA\n>long\n" + bases(_rng(11), L, b"ACGT") + b"\n>after\nGGT\n"
    return Case("fa-record-of-2^24%s-bases" % ("" if over else "-1"), make, 1, expect="back" if over else "taken", bit=A_LENGTHS if over else 0, size=L + 64,
                reach="DP_A_LENGTHS: a record of %d bases" % L)


# ---------------------------------------------------------------------------------------------
# all of them
# ---------------------------------------------------------------------------------------------
def _all():
    c = []
    for B in BORDERS:
        for o in OFFSETS:
            c += [fa_feature(f, B + o) for f in FA_FEATURES]
            c += [fq_feature(f, B + o) for f in FQ_FEATURES]
    for n in ENDS:
        for e in ENDINGS:
            if not (n == 1 and e == "crlf"):
                c.append(fa_end(n, e))
            if n >= 15:
                c.append(fq_end(n, e))
    c += [fa_long_seq(L, w) for L in (5000, 10000, 300000, 600000) for w in (False, True)]     # (5000: the state crosses a tile border; from 10000 on a whole tile is without a line start)
    c += [fa_long_header(5000), fa_long_header(10000), fa_long_header(300000), fa_two_long("header"), fa_two_long("sequence")]
    c += [fa_flush(e) for e in FLUSH_E]
    c += [fa_records(n, lead) for n in REC_COUNTS + (4097,) for lead in (False, True)]
    c += [fq_records(n, 33) for n in REC_COUNTS] + [fq_records(257, 64), fq_records(2049, 64)]
    c += [fa_flags(True, {r}, "N-in-%d" % r) for r in range(9)] + [fa_flags(False, {r}, "N-in-%d" % r) for r in range(1, 9)]
    c += [fa_flags(lead, {r, r + 1, r + 2, r + 3}, "N-in-%d-to-%d" % (r, r + 3)) for lead in (True, False) for r in range(0 if lead else 1, 6)]
    c += [fa_flags(True, set(), "none"), fa_flags(False, set(), "none")]
    c += [fa_scan2(), fa_limit(0), fa_limit(1)]
    names = [x.name for x in c]
    assert len(set(names)) == len(names)
    return c


CASES = _all()
SMALL = [x for x in CASES if not x.big]
LARGE = [x for x in CASES if x.big]
BY_NAME = {x.name: x for x in CASES}

_REF = {}
QUICK = 1 << 16


def reference(case, quick=False):
    """the serial reference of a case's text, made once (the vectorised one above BIG; quick: above QUICK too -- tests/test_dparse_cases_cpu.py
    holds the two against each other on every case below BIG, so a test that has a GPU to wait for need not walk 60 MB byte by byte again)"""
    from dparse_ref import parse, parse_vec
    if case.big:
        return parse_vec(case.text, case.fmt, case.qoff)
    key = (case.name, quick and len(case.text) > QUICK)
    if key not in _REF:
        _REF[key] = (parse_vec if key[1] else parse)(case.text, case.fmt, case.qoff)
    return _REF[key]
