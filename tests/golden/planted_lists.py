"""Planted buffers for the long-match-list rule sets (rules/lists31.yar, lists70.yar).

Deterministic like the generators of planted.py (CPython ``random`` + the
canonical xorshift), so tests/test_long_lists.py rebuilds the bytes that
make_lists.py scanned with stock libyara.
"""
import random

import numpy as np

from planted import _flip_case

# The atoms that dozens of strings share (4-byte lists of 31 .. 70 entries),
# the suffixes with lists of their own (`q9%`, `9%`: the shared tail of
# `#q9%`'s list) and the 1-byte keys with 4 .. 33 entries each.  The buffer
# begins with the first atom: its list holds two literals whose atom lies
# behind a prefix of zeros (backtrack 6 and 8), skipped at position 4
# (scanner.c:110), while the shared-tail entries (backtrack 3 and 2) are not.
LISTS = {
    "lists31": dict(atoms=[b"Zq9#"], tails=[], keys=b"~|^`"),
    "lists70": dict(atoms=[b"#q9%", b"Kx7!", b"Wm3&"], tails=[b"q9%", b"9%"], keys=b"~^|"),
}
# bytes before an atom: random ones (b""), a word character, a space, `_`, and
# the zeros of the prefixed literals
_LIST_PRE = [b"", b"", b" ", b"x", b"_", b"\x00\x00", b"\x00\x00\x00\x00", b"\x00"]
_LIST_LETTERS = b"ABCDEFabcdefGz-_ 4"


def lists_instances(name, r: random.Random):
    """One planted piece: (bytes, begin, end) with [begin, end) the atom or key
    in it.  An atom (a quarter of them with random letter case) after one of
    _LIST_PRE, followed by 0..8 zero bytes and a letter; or a 1-byte key alone
    or between alphanumerics, spaces or `_`."""
    spec = LISTS[name]
    x = r.random()
    if x < 0.7:
        pool = spec["atoms"] if (x < 0.55 or not spec["tails"]) else spec["tails"]
        a = r.choice(pool)
        if r.random() < 0.25:
            a = _flip_case(a, r)
        pre = r.choice(_LIST_PRE)
        tail = bytes(r.randint(0, 8)) + bytes([r.choice(_LIST_LETTERS)])
        return pre + a + tail, len(pre), len(pre) + len(a)
    k = bytes([r.choice(spec["keys"])])
    ctx = r.choice([(b"", b""), (b"a", b"b"), (b" ", b" "), (b"_", b"_"), (b"7", b" "), (b" ", b"Q")])
    return ctx[0] + k + ctx[1], len(ctx[0]), len(ctx[0]) + 1


def lists_layout(name, size: int, seed: int):
    """The planted pieces of lists_buffer: a list of (offset, bytes, begin, end)
    with [begin, end) the buffer range of the piece's atom or key."""
    spec = LISTS[name]
    r = random.Random(seed)
    head = spec["atoms"][0] + b"\x00\x00A"
    end = spec["atoms"][0] + bytes(3)     # cut by the buffer's end before its letter
    out = [(0, head, 0, 4)]
    pos = len(head)
    while True:
        pos += r.randint(1, 40)
        piece, a, b = lists_instances(name, r)
        if pos + len(piece) + 1 > size - len(end):
            break
        out.append((pos, piece, pos + a, pos + b))
        pos += len(piece)
    out.append((size - len(end), end, size - len(end), size - 3))
    return out


def lists_buffer(xorshift, name, size: int, seed: int) -> np.ndarray:
    """Random bytes with the shared atoms and 1-byte keys of a long-list rule
    set planted 1..40 bytes apart (long-list candidates on every lane of
    pre-verification's 64-candidate groups), an instance at the very start and
    one that the buffer's end cuts."""
    buf = xorshift(size, seed).copy()
    for off, piece, _, _ in lists_layout(name, size, seed):
        buf[off:off + len(piece)] = np.frombuffer(piece, dtype=np.uint8)
    return buf
