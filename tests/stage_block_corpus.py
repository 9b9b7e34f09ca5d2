"""Corpora for the chunk kernel's staging pass (stage_chunk, parse_chunk.h: a
lane takes one 64-byte mask block per round, a round is 4 KiB): small batches
that put line starts, terminators and chunk boundaries where that code can go
wrong.  Each builder returns the batch bytes; tests/test_stage_block.py
re-derives what a corpus claims to hold from its bytes (on the CPU), and
tests/test_stage_block_gpu.py runs the same corpora on the device.

A chunk is cb bytes, cb a multiple of 64 that depends on the batch's mean line
length and LP_OPT_CHUNK_LINES; a chunk's window starts 64 bytes before it, so
window blocks are the batch's 64-byte blocks.  The corpora therefore place
their features relative to EVERY multiple of 64 of a span longer than the
largest chunk (CB_MAX), so that a chunk boundary meets them whatever cb is."""
import random

CB_MIN, CB_MAX = 1024, 8192


def filler(n, i=0):
    """n bytes without a terminator, control byte, quote or byte >= 0x7F"""
    return (b"%d-" % i + b"abcdefghijklmnopqrstuvwxyz" * (n // 26 + 1))[:n]


class Batch:
    def __init__(self):
        self.parts = []
        self.n = 0

    def add(self, b):
        self.parts.append(b)
        self.n += len(b)

    def line(self, body, term=b"\n"):
        self.add(body + term)

    def align(self, residue, term=b"\n"):
        """a filler line whose terminator's last byte is just before the next offset = residue (mod 64)"""
        k = (residue - self.n - len(term)) % 64
        if k < 8:
            k += 64
        self.line(filler(k, self.n), term)
        assert self.n % 64 == residue

    def data(self):
        return b"".join(self.parts)


def line_starts(data):
    """start offsets of the batch's lines, byte by byte (Hadoop LineReader rules)"""
    starts, s, i, n = [], 0, 0, len(data)
    while i < n:
        c = data[i]
        if c in (0x0A, 0x0D):
            starts.append(s)
            if c == 0x0D and i + 1 < n and data[i + 1] == 0x0A:
                i += 1
            s = i + 1
        i += 1
    if s < n:
        starts.append(s)
    return starts


def terminators(data):
    """offsets of the bytes that end a line (the '\\n' of "\\r\\n", a lone '\\r', a '\\n')"""
    out = []
    for i, c in enumerate(data):
        if c == 0x0A or (c == 0x0D and not (i + 1 < len(data) and data[i + 1] == 0x0A)):
            out.append(i)
    return out


def block_counts(data):
    """terminators per 64-byte block"""
    out = [0] * ((len(data) + 63) // 64)
    for t in terminators(data):
        out[t // 64] += 1
    return out


def residues(base, reps=3):
    """line lengths 0..130 in turn (every start residue 0..63 of a block, starts
    and lines across every 1 KiB and 4 KiB mark), a real line every 9th"""
    b = Batch()
    k = 0
    for rep in range(reps):
        for n in range(131):
            b.line(filler(n, k))
            k += 1
            if k % 9 == 0:
                b.line(base[(k // 9) % len(base)])
    # a terminator in byte 63 of a block, the next line at byte 0 of the next
    for _ in range(4):
        b.align(0)
        b.line(base[_])
    return b.data()


DENSE_COUNTS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64)


def dense_starts(base):
    """blocks with k terminators for every k of DENSE_COUNTS (the rank's bit
    planes 0..6): k empty lines from byte 0 of a block, then a line that leaves
    the block; runs of 1-byte lines; 64 x '\\n' aligned and unaligned to a block"""
    b = Batch()
    for i, k in enumerate(DENSE_COUNTS):
        b.line(base[i % len(base)])
        b.align(0)
        b.add(b"\n" * k)
        if k < 64:
            b.line(filler(64 - k + 5, i))
    b.align(0)
    b.add(b"x\n" * 32)       # 32 one-byte lines: one block
    b.line(base[0])
    b.align(1)
    b.add(b"y\n" * 45)       # one-byte lines across blocks, odd phase
    b.line(base[1])
    b.align(60)
    b.add(b"tail")           # (its terminator is the run's first byte)
    b.add(b"\n" * 64)        # a whole block of terminators
    b.line(base[2])
    b.align(33)
    b.add(b"tail")
    b.add(b"\n" * 64)        # the same across two blocks
    b.line(base[3])
    b.align(0)
    b.add(b"\n" * 200)       # several whole blocks
    b.line(base[4])
    return b.data()


CR_BYTES = (15, 31, 47, 63)


def crlf(base):
    """"\\r\\n" with the '\\r' in byte 15, 31, 47 and 63 of a block (the '\\n' in
    the lane's next piece, or the next block), lone '\\r' at the same places and
    elsewhere, "\\r\\r", and '\\r' as the batch's last byte"""
    b = Batch()
    for rep in range(3):
        for i, cr in enumerate(CR_BYTES):
            b.line(base[(4 * rep + i) % len(base)], b"\r\n" if rep % 2 == 0 else b"\n")
            b.align((cr + 2) % 64, b"\r\n")          # "\r\n" with the '\r' at byte cr
            assert (b.n - 2) % 64 == cr
            b.line(filler(20 + i, i), b"\r")
            b.align((cr + 1) % 64, b"\r")            # a lone '\r' at byte cr, a filler byte after it
            b.line(filler(9, i), b"\r\n")
            b.align((cr + 1) % 64, b"\r")            # "\r\r": an empty line after the lone '\r' at byte cr
            b.add(b"\r")
    b.line(base[0], b"\r")                            # the batch ends in a lone '\r'
    return b.data()


def boundaries(base):
    """three spans, each longer than the largest chunk, of 64-byte periods: a
    '\\n' in byte 63 of every block (a chunk's t_lo, and the chunk before's
    t_hi), in byte 62 (t_hi - 1), in byte 0 (the byte after the boundary); so a
    chunk boundary falls just after, one past and just before a '\\n'"""
    b = Batch()
    for res in (0, 63, 1):
        b.line(base[res % len(base)])
        b.align(res)
        for k in range(2 * CB_MAX // 64 + 2):
            b.line(filler(63, k))
    b.line(base[5])
    return b.data()


def guard_lines(base, seed=5):
    """TAB and bytes >= 0x80 inside lines (the byte guard: `clean` windows and
    the others), among plain lines"""
    rng = random.Random(seed)
    out = []
    for i, l in enumerate(base):
        k = i % 4
        if k == 1:
            j = l.rindex(b'"', 0, len(l) - 1) + 1 + rng.randrange(3)
            l = l[:j] + b"\t" + l[j:]
        elif k == 2:
            j = l.rindex(b'"', 0, len(l) - 1) + 1 + rng.randrange(3)
            l = l[:j] + rng.choice(["é", "日本", "ü-x", " "]).encode() + l[j:]
        elif k == 3 and i % 8 == 3:
            l = l.replace(b" ", b"\t", 1)
        out.append(l)
    return b"".join(l + b"\n" for l in out)


def mixed(base, seed):
    """real lines of one log format with the staging corners between them: runs
    of empty and 1-byte lines (more than 64 starts in a chunk), "\\r\\n" and lone
    '\\r' terminators, a last line without a terminator"""
    rng = random.Random(seed)
    b = Batch()
    for i, l in enumerate(base):
        r = rng.random()
        b.line(l, b"\r\n" if r < 0.2 else b"\r" if r < 0.3 else b"\n")
        if i % 97 == 13:
            b.add(b"\n" * rng.randrange(5, 150))
        if i % 131 == 29:
            b.add(b"z\n" * rng.randrange(3, 90))
        if i % 53 == 7:
            b.align(rng.choice((0, 16, 32, 48)), b"\r\n")
    b.add(base[0])  # unterminated
    return b.data()
