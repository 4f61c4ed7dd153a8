"""A plain reference of the device read parser (metafast_amd/csrc/mf_dparse.hip), one byte at a time: no GPU, nothing of the library's.

It restates the rules at the head of mf_dparse.hip -- which are FastaReader's and FastqReader's, as oracle/mf_oracle.c (read_fasta, read_fastq)
has them -- in the form the kernels hand them on, so that every array of theirs can be compared, not only the last two:

  a line starts at byte 0 and behind every '\\n'; a '\\r' in front of a '\\n' (or as the text's last byte) belongs to the line's end, any other
  '\\r' is an anomaly (LONE_CR);
  FASTA  a line that starts with '>' or ';' is a header line and starts a record; record 0 is what stands in front of the first one, so
         n_rec = header lines + 1.  rec_seq[r] = nucleotide bytes (neither N nor a wrong character) in front of header line r, rec_seq[0] = 0,
         rec_seq[n_rec] = all of them; flag byte r: 1 = the record holds an N / n, 2 = it holds a character DnaTools.fromChar refuses.
         kept: at least one nucleotide and no N.  A wrong character without an N: BAD_CHAR; 2^24 nucleotides or more: LENGTHS.
         rec_place[r] = rec_seq[r] - (the place of the record's first base in the output): the nucleotides of dropped records in front of it.
  FASTQ  record r = lines 4 r .. 4 r + 3; ls[L] = first byte of line L, ls[n_lines] = n (n + 1 where the text does not end in '\\n': the line's
         end stands where the '\\n' would).  drop[r]: N / n / '.' in the sequence line or a quality character == qoff.  An empty line:
         EMPTY_LINE; another wrong character in a sequence line: BAD_CHAR; a quality outside [qoff, 126]: BAD_QUAL; lines 0 and 2 start
         with neither '@' nor '+': STRUCTURE; sequence and quality of different lengths, or none: LENGTHS.
         rec_place[r] = the place of the record's first base.
  both   rec_place of a dropped record and rec_place[n_rec] = DROP; offsets [kept + 1]; bases: upper-case A / C / G / T, IUPAC codes as their
         first listed base.

What the host does with the anomaly word is taken from dparse_kernels, not from what it returns: FASTA reads the word after pass 1 (only
LONE_CR can be in it) and returns there; pass 2 sets nothing; the record pass adds BAD_CHAR and LENGTHS and the word is read again.  FASTQ
reads it after pass 1 (LONE_CR, EMPTY_LINE), then returns without a bit if the lines are no multiple of four, and reads pass 2's bits
(BAD_CHAR, BAD_QUAL) together with the record pass's (STRUCTURE, LENGTHS).  `have` says how far it got: 0 = nothing to compare but the
word, 1 = the record arrays (rec_seq / flags, ls / drop), 2 = everything.

parse() is the serial form, parse_vec() the same rules over whole arrays for the texts of several MB (tests/test_dparse_cases_cpu.py
holds them against each other on every small case).  emit_pos (both): the text positions of the bytes that reach `bases`, in order."""
import numpy as np

A_LONE_CR, A_BAD_CHAR, A_EMPTY_LINE, A_BAD_QUAL, A_STRUCTURE, A_LENGTHS = 1, 2, 4, 8, 16, 32
BIT_NAMES = {1: "LONE_CR", 2: "BAD_CHAR", 4: "EMPTY_LINE", 8: "BAD_QUAL", 16: "STRUCTURE", 32: "LENGTHS"}
DROP = 0xFFFFFFFFFFFFFFFF
MAX_LEN = 1 << 24
NL, CR = 10, 13

# DnaTools.fromChar: 0 = refused, 0xFE = N / n, else the base
LUT = np.zeros(256, dtype=np.uint8)
for _src, _dst in zip(b"ACGTacgtRrYyMmKkSsWwHhBbVvDd", b"ACGTACGTGGTTAAGGGGAAAAGGAAAA"):
    LUT[_src] = _dst
LUT[ord("N")] = LUT[ord("n")] = 0xFE
_LUT = LUT.tolist()


class Parsed:
    """what the parser leaves: rc, anomaly, have, n_rec, n_lines; rec_a (rec_seq / ls), rec_b (flags / drop), keep, length, rec_place,
    offsets, bases, emit_pos; line_starts and header_lines (positions)"""

    def __init__(self, fmt):
        self.fmt, self.rc, self.anomaly, self.have, self.n_rec, self.n_lines = fmt, 1, 0, 0, 0, 0
        u64, u8 = np.uint64, np.uint8
        self.rec_a = self.rec_place = self.offsets = np.zeros(0, dtype=u64)
        self.rec_b = self.bases = np.zeros(0, dtype=u8)
        self.keep = np.zeros(0, dtype=bool)
        self.length = self.emit_pos = self.line_starts = self.header_lines = np.zeros(0, dtype=np.int64)

    def names(self):
        return [n for b, n in BIT_NAMES.items() if self.anomaly & b]


def _places(P, keep, length, rec_first):
    """keep / length per record -> rec_place, offsets (rec_first: FASTA's rec_seq, None for FASTQ)"""
    n_rec = len(keep)
    place = np.zeros(n_rec + 1, dtype=np.uint64)
    place[1:] = np.cumsum(np.where(keep, length, 0).astype(np.uint64))
    rp = np.full(n_rec + 1, DROP, dtype=np.uint64)
    k = np.flatnonzero(keep)
    rp[k] = place[k] if rec_first is None else rec_first[k] - place[k]
    P.keep, P.length, P.rec_place = keep, length, rp
    P.offsets = np.concatenate([place[k], place[-1:]])


def sniff_qoff(text):
    """ReadersUtils.determineQualityFormat on the first 1000 records, as the host does it before the kernels run: 64 unless a quality
    character (under a base that is no N / n / '.') is below 64 or above 126"""
    lines = text.replace(b"\r\n", b"\n").split(b"\n")
    for r in range(min(1000, len(lines) // 4)):
        s, q = lines[4 * r + 1], lines[4 * r + 3]
        for c, qc in zip(s, q):
            if c in b"Nn.":
                continue
            if qc < 64 or qc > 126:
                return 33
    return 64


# ---------------------------------------------------------------------------------------------
# serial
# ---------------------------------------------------------------------------------------------
def parse(text, fmt, qoff=33):
    t = bytes(text)
    assert len(t) >= 1 and fmt in (1, 2)
    return _fasta(t) if fmt == 1 else _fastq(t, qoff)


def _fasta(t):
    P = Parsed(1)
    n = len(t)
    lut = _LUT
    rec_seq, flags, starts, headers, seq_pos, seq_rec = [0], [0], [], [], [], []
    s = h = st = 0
    lone = False
    p = NL
    for i in range(n):
        c = t[i]
        if p == NL:
            starts.append(i)
            st = 1 if c == 62 or c == 59 else 0                 # '>' ';'
            if st:
                h += 1
                rec_seq.append(s)
                flags.append(0)
                headers.append(i)
        if c == CR:
            if (t[i + 1] if i + 1 < n else NL) != NL:
                lone = True
        elif c != NL and st == 0:
            v = lut[c]
            if v == 0xFE:
                flags[h] |= 1
            elif v == 0:
                flags[h] |= 2
            else:
                s += 1
                seq_pos.append(i)
                seq_rec.append(h)
        p = c
    P.line_starts, P.header_lines = np.array(starts, dtype=np.int64), np.array(headers, dtype=np.int64)
    if lone:
        P.anomaly = A_LONE_CR
        return P
    rec_seq.append(s)
    P.n_rec, P.have = h + 1, 1
    P.rec_a, P.rec_b = np.array(rec_seq, dtype=np.uint64), np.array(flags, dtype=np.uint8)
    keep, length = [], []
    for r in range(P.n_rec):
        ln, f = rec_seq[r + 1] - rec_seq[r], flags[r]
        length.append(ln)
        keep.append(ln > 0 and not f & 1)
        if f & 2 and not f & 1:
            P.anomaly |= A_BAD_CHAR
        if ln >= MAX_LEN:
            P.anomaly |= A_LENGTHS
    if P.anomaly:
        return P
    keep, length = np.array(keep, dtype=bool), np.array(length, dtype=np.int64)
    _places(P, keep, length, P.rec_a)
    pos, rec = np.array(seq_pos, dtype=np.int64), np.array(seq_rec, dtype=np.int64)
    P.emit_pos = pos[keep[rec]] if len(pos) else pos
    P.bases = LUT[np.frombuffer(t, dtype=np.uint8)[P.emit_pos]]
    P.rc, P.have = 0, 2
    return P


def _fastq(t, qoff):
    P = Parsed(2)
    n = len(t)
    lut = _LUT
    # pass 1
    nl = 0
    p = NL
    for i in range(n):
        c = t[i]
        if c == NL:
            nl += 1
            if p == NL:
                P.anomaly |= A_EMPTY_LINE
        elif c == CR:
            if (t[i + 1] if i + 1 < n else NL) != NL:
                P.anomaly |= A_LONE_CR
            elif p == NL:
                P.anomaly |= A_EMPTY_LINE
        p = c
    if P.anomaly:
        return P
    open_end = t[n - 1] != NL
    P.n_lines = nl + (1 if open_end else 0)
    if P.n_lines % 4:
        return P
    P.n_rec = P.n_lines // 4
    # pass 2
    ls, drop = [], [0] * P.n_rec
    line = 0
    p = NL
    bad = 0
    for i in range(n):
        c = t[i]
        if p == NL:
            ls.append(i)
        role = line & 3
        if c == NL:
            line += 1
        elif c != CR:
            if role == 1:
                if c == 78 or c == 110 or c == 46:              # 'N' 'n' '.'
                    drop[line >> 2] = 1
                elif lut[c] == 0 or lut[c] == 0xFE:
                    bad |= A_BAD_CHAR
            elif role == 3:
                if c < qoff or c > 126:
                    bad |= A_BAD_QUAL
                elif c == qoff:
                    drop[line >> 2] = 1
        p = c
    ls.append(n + 1 if open_end else n)
    assert len(ls) == P.n_lines + 1
    P.line_starts = np.array(ls[:-1], dtype=np.int64)
    P.header_lines = P.line_starts[0::4]
    P.rec_a, P.rec_b, P.have = np.array(ls, dtype=np.uint64), np.array(drop, dtype=np.uint8), 1
    # the records
    keep, length = [], []
    for r in range(P.n_rec):
        l0, l1, l2, l3, l4 = ls[4 * r:4 * r + 5]
        dl, ql = l2 - 1 - l1, l4 - 1 - l3
        if dl and t[l2 - 2] == CR:
            dl -= 1
        if ql and t[l4 - 2] == CR:
            ql -= 1
        if t[l0] not in b"@+" or t[l2] not in b"@+":
            bad |= A_STRUCTURE
        if dl != ql or dl == 0 or dl >= MAX_LEN:
            bad |= A_LENGTHS
        length.append(dl)
        keep.append(not drop[r])
    P.anomaly = bad
    if bad:
        return P
    keep, length = np.array(keep, dtype=bool), np.array(length, dtype=np.int64)
    _places(P, keep, length, None)
    pos = [np.arange(ls[4 * r + 1], ls[4 * r + 1] + length[r], dtype=np.int64) for r in range(P.n_rec) if keep[r]]
    P.emit_pos = np.concatenate(pos) if pos else np.zeros(0, dtype=np.int64)
    P.bases = LUT[np.frombuffer(t, dtype=np.uint8)[P.emit_pos]]
    P.rc, P.have = 0, 2
    return P


# ---------------------------------------------------------------------------------------------
# the same rules over whole arrays
# ---------------------------------------------------------------------------------------------
def parse_vec(text, fmt, qoff=33):
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    assert len(t) >= 1 and fmt in (1, 2)
    prev = np.concatenate([np.array([NL], dtype=np.uint8), t[:-1]])
    after = np.concatenate([t[1:], np.array([NL], dtype=np.uint8)])
    start = prev == NL
    lone = bool(np.any((t == CR) & (after != NL)))
    return _fasta_vec(t, start, lone) if fmt == 1 else _fastq_vec(t, prev, after, start, lone, qoff)


def _fasta_vec(t, start, lone):
    P = Parsed(1)
    P.line_starts = np.flatnonzero(start)
    hdr_start = start & ((t == 62) | (t == 59))
    P.header_lines = np.flatnonzero(hdr_start)
    if lone:
        P.anomaly = A_LONE_CR
        return P
    line_is_hdr = hdr_start[P.line_starts]
    in_hdr = line_is_hdr[np.cumsum(start) - 1]
    v = LUT[t]
    body = ~in_hdr & (t != NL) & (t != CR)
    base = body & (v != 0) & (v != 0xFE)
    rec = np.cumsum(hdr_start)                                   # the record of every byte
    n_rec = int(rec[-1]) + 1
    before = np.cumsum(base) - base                              # nucleotides in front of every byte
    rec_seq = np.zeros(n_rec + 1, dtype=np.uint64)
    rec_seq[1:n_rec] = before[P.header_lines]
    rec_seq[n_rec] = int(base.sum())
    flags = np.zeros(n_rec, dtype=np.uint8)
    flags[np.unique(rec[body & (v == 0xFE)])] |= 1
    flags[np.unique(rec[body & (v == 0)])] |= 2
    P.n_rec, P.have, P.rec_a, P.rec_b = n_rec, 1, rec_seq, flags
    length = np.diff(rec_seq.astype(np.int64))
    has_n = (flags & 1) != 0
    keep = (length > 0) & ~has_n
    if np.any(((flags & 2) != 0) & ~has_n):
        P.anomaly |= A_BAD_CHAR
    if np.any(length >= MAX_LEN):
        P.anomaly |= A_LENGTHS
    if P.anomaly:
        return P
    _places(P, keep, length, rec_seq)
    P.emit_pos = np.flatnonzero(base & keep[rec])
    P.bases = v[P.emit_pos]
    P.rc, P.have = 0, 2
    return P


def _fastq_vec(t, prev, after, start, lone, qoff):
    P = Parsed(2)
    n = len(t)
    is_nl = t == NL
    if lone:
        P.anomaly |= A_LONE_CR
    if np.any(is_nl & (prev == NL)) or np.any((t == CR) & (after == NL) & (prev == NL)):
        P.anomaly |= A_EMPTY_LINE
    if P.anomaly:
        return P
    open_end = t[-1] != NL
    P.n_lines = int(is_nl.sum()) + (1 if open_end else 0)
    if P.n_lines % 4:
        return P
    P.n_rec = n_rec = P.n_lines // 4
    P.line_starts = np.flatnonzero(start)
    P.header_lines = P.line_starts[0::4]
    ls = np.concatenate([P.line_starts, [n + 1 if open_end else n]]).astype(np.int64)
    line = np.cumsum(is_nl) - is_nl                              # the line of every byte (a '\n' belongs to the line it ends)
    role = line & 3
    body = ~is_nl & (t != CR)
    v = LUT[t]
    seq, qual = body & (role == 1), body & (role == 3)
    is_n = (t == 78) | (t == 110) | (t == 46)
    bad = 0
    if np.any(seq & ~is_n & ((v == 0) | (v == 0xFE))):
        bad |= A_BAD_CHAR
    if np.any(qual & ((t < qoff) | (t > 126))):
        bad |= A_BAD_QUAL
    drop = np.zeros(n_rec, dtype=np.uint8)
    drop[np.unique(line[seq & is_n] >> 2)] = 1
    drop[np.unique(line[qual & (t == qoff) & (t <= 126)] >> 2)] = 1
    P.rec_a, P.rec_b, P.have = ls.astype(np.uint64), drop, 1
    l0, l1, l2, l3, l4 = (ls[j:j + 4 * n_rec:4] for j in range(5))
    dl, ql = l2 - 1 - l1, l4 - 1 - l3
    dl = dl - ((dl > 0) & (t[np.maximum(l2 - 2, 0)] == CR))
    ql = ql - ((ql > 0) & (t[np.maximum(l4 - 2, 0)] == CR))
    ok_head = lambda c: (c == 64) | (c == 43)                    # '@' '+'
    if not (np.all(ok_head(t[l0])) and np.all(ok_head(t[l2]))):
        bad |= A_STRUCTURE
    if np.any((dl != ql) | (dl == 0) | (dl >= MAX_LEN)):
        bad |= A_LENGTHS
    P.anomaly = bad
    if bad:
        return P
    keep = drop == 0
    _places(P, keep, dl, None)
    P.emit_pos = np.flatnonzero(seq & keep[np.minimum(line >> 2, n_rec - 1)])
    P.bases = v[P.emit_pos]
    P.rc, P.have = 0, 2
    return P


ARRAYS = ("rec_a", "rec_b", "keep", "length", "rec_place", "offsets", "bases", "emit_pos", "line_starts", "header_lines")


def same(a, b):
    """-> the names of what differs between two Parsed"""
    out = [f for f in ("fmt", "rc", "anomaly", "have", "n_rec", "n_lines") if getattr(a, f) != getattr(b, f)]
    return out + [f for f in ARRAYS if not np.array_equal(np.asarray(getattr(a, f)).astype(np.int64, casting="unsafe") if f != "keep" else getattr(a, f),
                                                          np.asarray(getattr(b, f)).astype(np.int64, casting="unsafe") if f != "keep" else getattr(b, f))]
