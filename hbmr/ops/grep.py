"""Grep primitives (native/kernels/grep.hip) and their CPU twins.

The yardstick is :class:`hbmr.mapred.lib.basic.RegexMapper`: Python ``re`` over
the decoded line, ``finditer`` = leftmost-first (backtracking) matches, non
overlapping.  :func:`compile_pattern` turns the eligible subset of ``re``
syntax into a leftmost-first DFA:

* a Thompson NFA whose epsilon edges are ordered by priority (preferred branch
  first, greedy loops prefer the body, lazy loops the exit);
* DFA states are ordered tuples of NFA threads, cut after the first Match
  thread; a state accepts if its tuple ends in Match, and the last accepting
  position of a walk is the backtracking matcher's match end for that start;
* two start states (at line start / not), one synthetic end-of-line input
  class fed once at the line terminator so a trailing ``$`` can accept there.

A match table travels as ``(blob, counts)`` like a word table
(:mod:`hbmr.ops.text`), but its entries are split on ``\\n`` only: a match may
contain spaces.
"""
from __future__ import annotations

import collections
import re

import numpy as np
import torch

from . import _lib, text

try:                                    # Python ≥ 3.11
    from re import _constants as _C, _parser as _P
except ImportError:                     # pragma: no cover - older interpreters
    import sre_constants as _C
    import sre_parse as _P

MAX_STATES_KEY = "hbmr.grep.dfa.max.states"
MAX_STATES = 1024
TABLE_BYTES = 32 << 10                  # the transition table sits in LDS
MAX_COUNT = 16                          # largest n of {m,n}
WIDE_CLASS = 64
INITIAL_TABLE = 1 << 21                 # first match-table size tried (slots)

_ASCII = (1 << 128) - 1
_NL = 1 << 10
_CATEGORY = {}                          # sre category -> 128-bit member mask


class _Ineligible(Exception):
    pass


def _category_mask(cat):
    if not _CATEGORY:
        for name, esc in (("CATEGORY_DIGIT", r"\d"), ("CATEGORY_NOT_DIGIT", r"\D"),
                          ("CATEGORY_SPACE", r"\s"), ("CATEGORY_NOT_SPACE", r"\S"),
                          ("CATEGORY_WORD", r"\w"), ("CATEGORY_NOT_WORD", r"\W")):
            rx = re.compile(esc)
            _CATEGORY[getattr(_C, name)] = sum(1 << c for c in range(128) if rx.match(chr(c)))
    if cat not in _CATEGORY:
        raise _Ineligible(f"character category {cat} is not supported on the GPU")
    return _CATEGORY[cat]


def _ascii(c):
    if c >= 128:
        raise _Ineligible("non-ASCII literal: the GPU matcher works on bytes")
    return c


def _class_mask(items):
    neg = False
    m = 0
    for op, av in items:
        if op is _C.NEGATE:
            neg = True
        elif op is _C.LITERAL:
            m |= 1 << _ascii(av)
        elif op is _C.RANGE:
            lo, hi = av
            _ascii(hi)
            m |= ((1 << (hi + 1)) - 1) & ~((1 << lo) - 1)
        elif op is _C.CATEGORY:
            m |= _category_mask(av)
        else:
            raise _Ineligible(f"class item {op} is not supported on the GPU")
    return (~m & _ASCII) if neg else m


def _single_mask(op, av):
    """Member mask of a one-character item, else None."""
    if op is _C.LITERAL:
        return 1 << _ascii(av)
    if op is _C.NOT_LITERAL:
        return _ASCII & ~(1 << _ascii(av))
    if op is _C.ANY:
        return _ASCII
    if op is _C.IN:
        return _class_mask(av)
    return None


class _Nfa:
    """Nodes: ("char", mask, out) | ("eol", out) | ("split", first, second) |
    ("match",).  Built back to front: every builder takes the continuation."""

    def __init__(self):
        self.nodes = [("match",)]

    def add(self, *node):
        self.nodes.append(node)
        return len(self.nodes) - 1

    def seq(self, items, nxt):
        for op, av in reversed(list(items)):
            nxt = self.item(op, av, nxt)
        return nxt

    def item(self, op, av, nxt):
        m = _single_mask(op, av)
        if m is not None:
            return self.add("char", m & ~_NL, nxt)      # a line holds no '\n'
        if op is _C.BRANCH:
            alts = [self.seq(a, nxt) for a in av[1]]
            cur = alts[-1]
            for a in reversed(alts[:-1]):
                cur = self.add("split", a, cur)
            return cur
        if op is _C.SUBPATTERN:
            _, add_flags, del_flags, p = av
            if add_flags or del_flags:
                raise _Ineligible("inline flags are not supported on the GPU")
            return self.seq(p, nxt)
        if op in (_C.MAX_REPEAT, _C.MIN_REPEAT):
            lo, hi, p = av
            greedy = op is _C.MAX_REPEAT
            unbounded = hi == _C.MAXREPEAT
            if lo > MAX_COUNT or (not unbounded and hi > MAX_COUNT):
                raise _Ineligible(f"repeat count above {MAX_COUNT}")
            if unbounded:
                loop = self.add("split", 0, 0)
                body = self.seq(p, loop)
                self.nodes[loop] = ("split", body, nxt) if greedy else ("split", nxt, body)
                cur = loop
            else:
                cur = nxt
                for _ in range(hi - lo):
                    body = self.seq(p, cur)
                    cur = self.add("split", body, nxt) if greedy else self.add("split", nxt, body)
            for _ in range(lo):
                cur = self.seq(p, cur)
            return cur
        if op is _C.AT:
            raise _Ineligible("only a leading ^ and a trailing $ are supported on the GPU "
                              f"({str(av).lower()} elsewhere in the pattern)")
        if op in (_C.GROUPREF, _C.GROUPREF_EXISTS):
            raise _Ineligible("back-references need a backtracking matcher")
        if op in (_C.ASSERT, _C.ASSERT_NOT):
            raise _Ineligible("look-around is not supported on the GPU")
        raise _Ineligible(f"{str(op).lower()} is not supported on the GPU")


class GrepProgram:
    """A compiled pattern: ``byteclass[256]`` uint8 (bytes ≥ 0x80 and ``\\n``
    → class 0, the dead class), ``trans[nstates, nclasses]`` uint16 (state 0
    dead, last class = end of line), ``accept[nstates]`` uint8, the two start
    states."""

    def __init__(self, regex, byteclass, trans, accept, start_bol, start_mid):
        self.regex = regex
        self.group = 0
        self.byteclass = byteclass
        self.trans = trans
        self.accept = accept
        self.nstates, self.nclasses = trans.shape
        self.start_bol = int(start_bol)
        self.start_mid = int(start_mid)
        self._device = {}

    def device_table(self):
        """The kernels' table: next state, bit 15 set if that state accepts."""
        return (self.trans | (self.accept[self.trans].astype(np.uint16) << 15)).astype(np.uint16)

    def on_device(self, device, stream=None):
        """(table, byteclass) tensors on ``device``, uploaded on the calling
        stream and cached per (device, stream): a cache shared between streams
        would let a second stream read the tables before the first stream's
        copy has landed."""
        s = torch.cuda.current_stream(device) if stream is None else stream
        key = (str(device), int(s.cuda_stream))
        got = self._device.get(key)
        if got is None:
            with torch.cuda.stream(s):
                tab = torch.from_numpy(self.device_table().view(np.int16).reshape(-1)).to(device)
                cls = torch.from_numpy(self.byteclass.copy()).to(device)
            got = self._device[key] = (tab, cls)
        return got


def _first_atoms(items):
    """The items a match can begin with (through groups and alternatives)."""
    items = list(items)
    if not items:
        return
    op, av = items[0]
    if op is _C.SUBPATTERN:
        yield from _first_atoms(av[3])
    elif op is _C.BRANCH:
        for a in av[1]:
            yield from _first_atoms(a)
    else:
        yield op, av


def _check_cost(items):
    for op, av in _first_atoms(items):
        if op in (_C.MAX_REPEAT, _C.MIN_REPEAT) and av[1] == _C.MAXREPEAT and len(av[2]) == 1:
            m = _single_mask(*av[2][0])
            # a wide class that holds the space is not stopped by word breaks:
            # every start offset walks to the line end
            if m is not None and bin(m & ~_NL).count("1") >= WIDE_CLASS and m >> 32 & 1:
                raise _Ineligible(
                    "the pattern starts with an unbounded repeat of a class with "
                    f">= {WIDE_CLASS} members: each start offset walks its own match, "
                    "so that costs O(line length squared)")


def _compile(regex, group, max_states):
    if group != 0:
        raise _Ineligible("only group 0 is matched on the GPU")
    try:
        parsed = _P.parse(regex)
    except Exception as e:  # noqa: BLE001 - re.error, RecursionError, ...
        raise _Ineligible(f"cannot parse pattern: {e}")
    flags = getattr(parsed, "state", getattr(parsed, "pattern", None)).flags
    if flags & ~_C.SRE_FLAG_UNICODE:
        raise _Ineligible("inline flags are not supported on the GPU")
    items = list(parsed)
    anchored = bool(items) and items[0] == (_C.AT, _C.AT_BEGINNING)
    if anchored:
        items = items[1:]
    dollar = bool(items) and items[-1] == (_C.AT, _C.AT_END)
    if dollar:
        items = items[:-1]
    _check_cost(items)
    nfa = _Nfa()
    tail = nfa.add("eol", 0) if dollar else 0
    start = nfa.seq(items, tail)
    nodes = nfa.nodes

    def closure(n, out, seen):
        """Threads reachable from n by epsilon edges, in priority order;
        True once Match is reached (lower-priority threads are cut)."""
        stack = [n]
        while stack:
            n = stack.pop()
            if n in seen:
                continue
            seen.add(n)
            node = nodes[n]
            if node[0] == "split":
                stack.append(node[2])
                stack.append(node[1])
            else:
                out.append(n)
                if node[0] == "match":
                    return True
        return False

    first, seen = [], set()
    closure(start, first, seen)
    first = tuple(first)
    if first and nodes[first[-1]][0] == "match":
        raise _Ineligible("the pattern can match the empty string")

    # byte classes: bytes with the same membership in every char node
    masks = sorted({nd[1] for nd in nodes if nd[0] == "char"})
    sig_class = {}
    byteclass = np.zeros(256, dtype=np.uint8)
    reps = [None]                          # class -> a representative byte (0: dead)
    for c in range(128):
        sig = tuple(m >> c & 1 for m in masks)
        if not any(sig):
            continue
        if sig not in sig_class:
            sig_class[sig] = len(reps)
            reps.append(c)
        byteclass[c] = sig_class[sig]
    eol = len(reps)
    ncls = eol + 1
    if ncls > 255:
        raise _Ineligible("too many byte classes")

    def step(state, cls):
        out, seen = [], set()
        for n in state:
            node = nodes[n]
            if node[0] == "char":
                hit = cls != eol and node[1] >> reps[cls] & 1
            elif node[0] == "eol":
                hit = cls == eol
            else:
                break                       # Match: the tuple ends here
            if hit and closure(node[-1], out, seen):
                break
        return tuple(out)

    ids = {(): 0, first: 1}
    order = [(), first]
    rows = [[0] * ncls]
    i = 1
    while i < len(order):
        row = [0] * ncls
        for cls in range(1, ncls):
            nxt = step(order[i], cls)
            if nxt not in ids:
                ids[nxt] = len(order)
                order.append(nxt)
                if len(order) > max_states:
                    raise _Ineligible(f"the DFA needs more than {max_states} states "
                                      f"({MAX_STATES_KEY})")
                if len(order) * ncls * 2 > TABLE_BYTES:
                    raise _Ineligible(f"the DFA table is larger than {TABLE_BYTES >> 10} KiB "
                                      "of LDS")
            row[cls] = ids[nxt]
        rows.append(row)
        i += 1
    trans = np.array(rows, dtype=np.uint16)
    accept = np.array([1 if s and nodes[s[-1]][0] == "match" else 0 for s in order],
                      dtype=np.uint8)
    if accept[trans[1, eol]]:
        raise _Ineligible("the pattern can match the empty string")
    return GrepProgram(regex, byteclass, trans, accept, 1, 0 if anchored else 1)


_REASONS = {}


def compile_pattern(regex: str, group: int = 0, max_states: int = MAX_STATES):
    """The pattern's :class:`GrepProgram`, or None if it is not eligible for
    the GPU (:func:`why_ineligible` gives the reason)."""
    try:
        prog = _compile(regex, group, max_states)
        _REASONS.pop((regex, group), None)
        return prog
    except _Ineligible as e:
        _REASONS[(regex, group)] = str(e)
        return None


def why_ineligible(regex: str, group: int = 0, max_states: int = MAX_STATES):
    """Why :func:`compile_pattern` refuses the pattern (None if it does not)."""
    compile_pattern(regex, group, max_states)
    return _REASONS.get((regex, group))


# --------------------------------------------------------------------------- CPU twins
def _candidates(prog, data: bytes):
    """(pos, len) of every start offset with a match: a walk of the table."""
    a = np.frombuffer(data, dtype=np.uint8)
    n = len(a)
    cls = prog.byteclass[a] if n else a
    nl = a == 10
    nxt_nl = np.ones(n, dtype=bool)
    nxt_nl[:-1] = nl[1:]
    term = (nl | ((a == 13) & nxt_nl)).tolist()
    cls = cls.tolist()
    trans = prog.trans.tolist()
    accept = prog.accept.tolist()
    eol = prog.nclasses - 1
    out = []
    for i in range(n):
        st = prog.start_bol if i == 0 or data[i - 1] == 10 else prog.start_mid
        best, t = 0, i
        while st:
            if t >= n or term[t]:
                if accept[trans[st][eol]]:
                    best = t - i
                break
            st = trans[st][cls[t]]
            t += 1
            if accept[st]:
                best = t - i
        if best:
            out.append((i, best))
    return out


def _select(cands):
    """finditer's non-overlapping choice: a greedy chain over the candidates."""
    out, end = [], 0
    for p, ln in cands:
        if p >= end:
            out.append((p, ln))
            end = p + ln
    return out


def simulate(prog, data: bytes) -> list:
    """``(start, len)`` of the matches ``re.finditer`` finds line by line, from
    the same tables the kernels walk."""
    return _select(_candidates(prog, data))


def split_lines(data: bytes) -> list:
    """The lines LineRecordReader returns for a buffer of whole lines."""
    lines = data.split(b"\n")
    if lines and not lines[-1]:
        lines.pop()
    return [ln[:-1] if ln.endswith(b"\r") else ln for ln in lines]


def count_matches_cpu(data: bytes, regex: str, group: int = 0):
    """RegexMapper + combiner over a split's bytes → (blob, counts)."""
    rx = re.compile(regex)
    c = collections.Counter()
    for ln in split_lines(data):
        for m in rx.finditer(ln.decode("utf-8", errors="replace")):
            c[m.group(group).encode("utf-8")] += 1
    return text._table_from(c)


def merge_tables_cpu(blob: bytes, counts, R: int = 1):
    """Sum a concatenation of match tables (entries end at ``\\n``)."""
    return text.merge_tables_cpu(blob, counts, R)


# --------------------------------------------------------------------------- GPU
_ptr, _st, _call = text._ptr, text._st, text._call


def candidates(buf, prog, stream=None):
    """(pos, len int32, end int64, non_ascii) of every start offset of the
    aligned device buffer with a match, in position order."""
    n = buf.numel()
    dev = buf.device
    if int(prog.trans.max()) >= prog.nstates or int(prog.byteclass.max()) >= prog.nclasses:
        raise ValueError("corrupt DFA table")       # the kernel indexes LDS with these
    tab, cls = prog.on_device(dev, stream)
    dfa = (_ptr(tab), _ptr(cls), prog.nstates, prog.nclasses, prog.start_bol, prog.start_mid)
    tiles = _lib.load().hbmr_wc_tiles(n)
    tc = torch.empty(tiles, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    _call("hbmr_grep_cand_count", _ptr(buf), n, *dfa, _ptr(tc), _ptr(flag), _st(stream))
    base, nc = text._tile_scan(tc)
    pos = torch.empty(nc, dtype=torch.int32, device=dev)
    ln = torch.empty(nc, dtype=torch.int32, device=dev)
    end = torch.empty(nc, dtype=torch.int64, device=dev)
    if nc:
        _call("hbmr_grep_cand_write", _ptr(buf), n, *dfa, _ptr(base), _ptr(pos), _ptr(ln),
              _ptr(end), _st(stream))
    return pos, ln, end, bool(int(flag))


def select(pos, ln, end, stream=None):
    """The candidates finditer keeps (non-overlapping, leftmost), in order."""
    nc = pos.numel()
    if nc == 0:
        return pos, ln
    dev = pos.device
    blocks = _lib.load().hbmr_grep_select_blocks(nc)
    # running maximum of the ends: per-block maxima, their scan here, the rewrite
    bmax = torch.empty(blocks, dtype=torch.int64, device=dev)
    _call("hbmr_grep_block_max", _ptr(end), nc, _ptr(bmax), _st(stream))
    bpre = torch.zeros(blocks, dtype=torch.int64, device=dev)
    if blocks > 1:
        bpre[1:] = torch.cummax(bmax, 0).values[:-1]
    pmax = torch.empty(nc, dtype=torch.int64, device=dev)
    _call("hbmr_grep_prefix_max", _ptr(end), nc, _ptr(bpre), _ptr(pmax), _st(stream))
    bc = torch.empty(blocks, dtype=torch.int32, device=dev)
    _call("hbmr_grep_select_count", _ptr(pos), _ptr(ln), _ptr(pmax), nc, _ptr(bc), _st(stream))
    base, ns = text._tile_scan(bc)
    spos = torch.empty(ns, dtype=torch.int32, device=dev)
    slen = torch.empty(ns, dtype=torch.int32, device=dev)
    _call("hbmr_grep_select_write", _ptr(pos), _ptr(ln), _ptr(pmax), nc, _ptr(base), _ptr(spos),
          _ptr(slen), _st(stream))
    return spos, slen


def aggregate(buf, starts, lens, weights=None, R=1, stream=None):
    """Exact per-span totals: (ustart, ulen, ucount int64, upart int32), unordered.
    ``upart`` = (Text.hashCode() & INT_MAX) % R (Hadoop's HashPartitioner)."""
    compact = ("hbmr_span_compact", _ptr(buf), _ptr(starts), _ptr(lens))
    return text._aggregate("hbmr_span_insert", compact, ("match", "matches"), INITIAL_TABLE, buf,
                           starts, lens, weights, R, stream)


def lines(blob, stream=None):
    """(start, len) int32 pairs of the ``\\n``-terminated entries of a blob."""
    return text._itemize("hbmr_lines_count", "hbmr_lines_write", blob, stream)


def count_matches(buf: torch.Tensor, prog: GrepProgram, stream=None):
    """Map + combine of one text split → (blob, counts, non_ascii).  With
    ``non_ascii`` set the split holds a byte ≥ 0x80 and the table is not
    RegexMapper's (``re`` sees decoded text there): map it with
    :func:`count_matches_cpu`."""
    if buf.device.type != "cuda":
        data = bytes(buf.numpy())
        blob, counts = count_matches_cpu(data, prog.regex, prog.group)
        return blob, counts, max(data, default=0) >= 0x80
    if buf.numel() == 0:
        return (torch.empty(0, dtype=torch.uint8, device=buf.device),
                torch.empty(0, dtype=torch.int64, device=buf.device), False)
    buf = text._aligned(buf.contiguous())
    pos, ln, end, non_ascii = candidates(buf, prog, stream)
    spos, slen = select(pos, ln, end, stream)
    us, ul, uc, _ = aggregate(buf, spos, slen, None, 1, stream)
    return text.pack(buf, us, ul, None, stream), uc, non_ascii


def merge_tables(blob: torch.Tensor, counts: torch.Tensor, R: int = 1, stream=None):
    """:func:`hbmr.ops.text.merge_tables` for match tables: entries end at
    ``\\n`` only.  Returns (blob, counts, part_bytes, part_words)."""
    if blob.device.type != "cuda":
        return merge_tables_cpu(bytes(blob.numpy()), counts, R)
    return text._merge(lines, aggregate, ("match", "entries"), text._aligned(blob.contiguous()),
                       counts, R, stream)
