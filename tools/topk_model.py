"""Executable model of the HIP top-k (mx_quantization_amd/csrc/mxa_topk.hip).

It reproduces torch's CPU `topk(largest=True, sorted=True)` index order
(TopKImpl.h:45-86 -> libstdc++ 11 nth_element + sort, or partial_sort when
k*64 <= n) WITHOUT running the serial algorithms element by element: every
Hoare partition step is computed from per-position flags and prefix counts,
which is what one wavefront does with ballots (SURVEY.md §7 "Hard parts").

Partition of [first, last) around the pivot p at `first` (stl_algo.h
__unguarded_partition, with comp(x, y) = x > y):
  left stop  x in [first+1, last):  !(a[x] > p)
  right stop y in [first, last):    !(p > a[y])
  A(x)   = # left stops  at positions < x      (rank of a left stop)
  Bgt(y) = # right stops at positions > y      (rank of a right stop)
  left stop x swaps  iff Bgt(x) > A(x);  right stop y swaps iff A(y) > Bgt(y)
  the t-th swapping left stop exchanges with the t-th swapping right stop
  cut = min(first non-swapping left stop, lowest swapping right stop)
        (lowest swapping right stop := last when nothing swaps)

std::sort's final insertion sort is a stable sort; because introsort leaves
segments of <= 16 elements that are mutually ordered, it equals a stable sort
of each segment.  The depth-limit fallbacks (heap_select / heapsort) and the
partial_sort branch are serial in the kernel too; here they are restated from
stl_heap.h.

`partition_lanes` is the same step in the form the row-group kernel computes it
(mxa_topk_grp.hpp grp_partition: 16 lanes of E positions, one slot index space for
both kinds of swapping stop); `Row(keys, lanes=True)` runs the whole top-k on it.

Used by tests/test_topk_model.py to check the model against oracle/topk_ref.cpp and
by tests/test_exchange_model_cpu.py to check the lane form against the reference form.
"""
from __future__ import annotations

import numpy as np


def keys_from_f32(x: np.ndarray) -> np.ndarray:
    """Order-preserving uint32 keys for torch's comparator: NaN largest (all NaNs
    equal), -0 == +0."""
    x = np.asarray(x, dtype=np.float32).copy()
    x[x == 0] = 0.0
    b = x.view(np.uint32).astype(np.uint64)
    k = np.where(b >> 31, (~b) & 0xFFFFFFFF, b | 0x80000000)
    k = np.where(np.isnan(x), 0xFFFFFFFF, k)
    return k.astype(np.uint64)


def lg(n: int) -> int:
    return n.bit_length() - 1


LANES = 16  # one DPP row per top-k row (mxa_topk_grp.hpp)
WIDTHS = (2, 4, 6, 8, 10, 12, 14, 16, 24, 32)  # grp_partition_any's window widths E


def popc(x: int) -> int:
    return bin(x).count("1")


def lowbits(n: int) -> int:
    return (1 << n) - 1


def grp_alloc(n: int) -> int:
    """mxa_topk_grp.hpp grp_alloc: the mirror's allocated positions."""
    return (n + 31) & ~31 if n <= 256 else (384 if n <= 384 else 512)


def window_for(n: int, f: int, l: int):
    """(E, b) of grp_partition_any for the range [f, l) of an n-key row (n <= 512): the
    narrowest 16 E positions from an even base at or below f that hold the range."""
    assert n <= 512
    npa = grp_alloc(n)
    need = l - (f & ~1)
    for E in WIDTHS:
        if LANES * E <= npa and need <= LANES * E:
            return E, min(f & ~1, npa - LANES * E)
    raise ValueError((n, f, l))


def partition_lanes(keys, f, l, E, b, idx=None):
    """One partition step as grp_partition (mxa_topk_grp.hpp) computes it: 16 lanes of E
    positions from base b (b <= f, l <= b + 16 E); lane g holds positions b + E g + e, bit
    E-1-e of its masks.  The median step first (as __unguarded_partition_pivot), then per
    lane: stop masks Lm / Rm, prefix counts PL / PR over the lower lanes, the prefix length
    j of its positions below the cut, its swapping left stops SLm (the left stops of those
    j positions) and its swapping right stops SRm (its cS highest-position right stops,
    the cS lowest set bits of Rm), X = SLm | SRm.  Along the row every swapping left stop
    precedes every swapping right stop, so ONE slot index space serves both: the slot of a
    set bit of X is base + the set bits of X before it in the lane, base = PL where the lane
    has positions below the cut, else nsw + the swapping right stops of the lower lanes.
    Left stops fill [0, nsw), right stops [nsw, 2 nsw), both in position order; the t-th
    pair is slot[t] <-> slot[2 nsw - 1 - t].
    Returns (keys, idx, cut, info): the arrays after the step and info = {nsw, slots (the
    slot table as a dict), X (the lanes' combined masks), j (the lanes' prefix lengths)}."""
    k = np.array(keys, dtype=np.uint64)
    i = np.arange(len(k), dtype=np.int64) if idx is None else np.array(idx, dtype=np.int64)
    assert b <= f and l <= b + LANES * E and l - f >= 3
    r = Row(k)
    r.i = i
    r.median_to_first(f, l)
    k, i = r.k, r.i
    p = int(k[f])
    Lm, Rm = [0] * LANES, [0] * LANES
    for g in range(LANES):
        for e in range(E):
            z = b + E * g + e
            if f + 1 <= z < l:  # the pivot position never counts, nor the window's padding
                Lm[g] |= (int(k[z]) <= p) << (E - 1 - e)
                Rm[g] |= (int(k[z]) >= p) << (E - 1 - e)
    cntL, cntR = [popc(x) for x in Lm], [popc(x) for x in Rm]
    PL = [sum(cntL[:g]) for g in range(LANES)]
    PR = [sum(cntR[:g]) for g in range(LANES)]
    totR = sum(cntR)
    # the cut: per lane the longest prefix of its positions with T(z) <= totR
    j = []
    for g in range(LANES):
        c = 0
        while c < E and PL[g] + PR[g] + popc(Lm[g] >> (E - c - 1)) + popc(Rm[g] >> (E - c - 1)) <= totR:
            c += 1
        j.append(c)
    SLm = [Lm[g] & ~lowbits(E - j[g]) for g in range(LANES)]
    cut = b + sum(j)
    nsw = sum(popc(x) for x in SLm)
    X, base = [], []
    for g in range(LANES):
        here_up = totR - PR[g]  # right stops in this lane and above
        cS = min(max(nsw - (here_up - cntR[g]), 0), cntR[g])
        w = 0  # largest prefix (from the low bits: the highest positions) with <= cS right stops
        while w < E and popc(Rm[g] & lowbits(w + 1)) <= cS:
            w += 1
        SRm = Rm[g] & lowbits(w)
        assert popc(SRm) == cS and SLm[g] & SRm == 0
        X.append(SLm[g] | SRm)
        base.append(PL[g] if j[g] > 0 else 2 * nsw - min(nsw, here_up))
    slots = {}
    for g in range(LANES):
        for e in range(E):
            sh = E - 1 - e
            if (X[g] >> sh) & 1:
                s = base[g] + popc((X[g] >> sh) >> 1)
                assert s not in slots
                slots[s] = b + E * g + e
    kk, ii = k.copy(), i.copy()
    for t in range(nsw):
        x, y = slots[t], slots[2 * nsw - 1 - t]
        k[x], k[y] = kk[y], kk[x]
        i[x], i[y] = ii[y], ii[x]
    return k, i, cut, {"nsw": nsw, "slots": slots, "X": X, "j": j}


class Row:
    def __init__(self, keys, lanes=False):
        """lanes: every partition step runs in the lane form (partition_lanes, in the
        window grp_partition_any picks) instead of the reference form partition_pivot."""
        self.k = np.array(keys, dtype=np.uint64)
        self.i = np.arange(len(keys), dtype=np.int64)
        self.fallbacks = 0
        self.lanes = lanes

    def gt(self, a, b):  # comp(a, b) on positions
        return self.k[a] > self.k[b]

    def swap(self, a, b):
        self.k[[a, b]] = self.k[[b, a]]
        self.i[[a, b]] = self.i[[b, a]]

    def median_to_first(self, first, last):
        """__move_median_to_first(first, first + 1, mid, last - 1)"""
        mid = first + (last - first) // 2
        a, b, c = first + 1, mid, last - 1
        if self.gt(a, b):
            if self.gt(b, c):
                self.swap(first, b)
            elif self.gt(a, c):
                self.swap(first, c)
            else:
                self.swap(first, a)
        elif self.gt(a, c):
            self.swap(first, a)
        elif self.gt(b, c):
            self.swap(first, c)
        else:
            self.swap(first, b)

    # -- parallel-rule partition -------------------------------------------------
    def partition(self, first, last):
        """One __unguarded_partition_pivot step in the form the row was built for."""
        if not self.lanes:
            return self.partition_pivot(first, last)
        E, b = window_for(len(self.k), first, last)
        self.k, self.i, cut, _ = partition_lanes(self.k, first, last, E, b, self.i)
        return cut

    def partition_pivot(self, first, last):
        self.median_to_first(first, last)
        p = self.k[first]
        pos = np.arange(first, last)
        seg = self.k[first:last]
        lstop = (seg <= p) & (pos >= first + 1)
        rstop = seg >= p
        A = np.cumsum(lstop) - lstop  # exclusive prefix
        Bgt = rstop[::-1].cumsum()[::-1] - rstop
        swl = lstop & (Bgt > A)
        swr = rstop & (A > Bgt)
        m = int(swl.sum())
        assert m == int(swr.sum())
        lpos = pos[swl]  # ascending: rank t = A
        rpos = pos[swr][::-1]  # descending: rank t = Bgt
        kk, ii = self.k.copy(), self.i.copy()
        self.k[lpos], self.k[rpos] = kk[rpos], kk[lpos]
        self.i[lpos], self.i[rpos] = ii[rpos], ii[lpos]
        nl = pos[lstop & ~swl]
        c1 = int(nl[0]) if len(nl) else 1 << 30
        c2 = int(rpos[-1]) if m else last
        return min(c1, c2)

    def stable_sort(self, first, last):
        if last - first < 2:
            return
        o = np.argsort(-self.k[first:last].astype(np.float64), kind="stable")
        self.k[first:last] = self.k[first:last][o]
        self.i[first:last] = self.i[first:last][o]

    # -- serial heap algorithms (stl_heap.h) ---------------------------------------
    def _push_heap(self, base, hole, top, vk, vi):
        parent = (hole - 1) // 2
        while hole > top and self.k[base + parent] > vk:
            self.k[base + hole], self.i[base + hole] = self.k[base + parent], self.i[base + parent]
            hole = parent
            parent = (hole - 1) // 2
        self.k[base + hole], self.i[base + hole] = vk, vi

    def _adjust_heap(self, base, hole, ln, vk, vi):
        top = hole
        second = hole
        while second < (ln - 1) // 2:
            second = 2 * (second + 1)
            if self.k[base + second] > self.k[base + second - 1]:
                second -= 1
            self.k[base + hole], self.i[base + hole] = self.k[base + second], self.i[base + second]
            hole = second
        if (ln & 1) == 0 and second == (ln - 2) // 2:
            second = 2 * (second + 1)
            self.k[base + hole], self.i[base + hole] = self.k[base + second - 1], self.i[base + second - 1]
            hole = second - 1
        self._push_heap(base, hole, top, vk, vi)

    def _make_heap(self, first, last):
        ln = last - first
        if ln < 2:
            return
        parent = (ln - 2) // 2
        while True:
            self._adjust_heap(first, parent, ln, self.k[first + parent], self.i[first + parent])
            if parent == 0:
                return
            parent -= 1

    def _pop_heap(self, first, last, result):
        vk, vi = self.k[result], self.i[result]
        self.k[result], self.i[result] = self.k[first], self.i[first]
        self._adjust_heap(first, 0, last - first, vk, vi)

    def heap_select(self, first, middle, last):
        self._make_heap(first, middle)
        for i in range(middle, last):
            if self.k[i] > self.k[first]:
                self._pop_heap(first, middle, i)

    def sort_heap(self, first, last):
        while last - first > 1:
            last -= 1
            self._pop_heap(first, last, last)

    # -- algorithms -------------------------------------------------------------
    def nth_element(self, nth, first=0, last=None):
        last = len(self.k) if last is None else last
        if first == last or nth == last:
            return
        depth = 2 * lg(last - first)
        while last - first > 3:
            if depth == 0:
                self.fallbacks += 1
                self.heap_select(first, nth + 1, last)
                self.swap(first, nth)
                return
            depth -= 1
            cut = self.partition(first, last)
            if cut <= nth:
                first = cut
            else:
                last = cut
        self.stable_sort(first, last)

    def sort(self, first, last):
        if first == last:
            return
        stack = [(first, last, 2 * lg(last - first))]
        while stack:  # segment order is irrelevant: segments are disjoint
            f, l, depth = stack.pop()
            while l - f > 16:
                if depth == 0:
                    self.fallbacks += 1
                    self.heap_select(f, l, l)
                    self.sort_heap(f, l)
                    l = f  # segment finished (heapsort is a full sort)
                    break
                depth -= 1
                cut = self.partition(f, l)
                stack.append((cut, l, depth))
                l = cut
            if l > f:
                self.stable_sort(f, l)

    def partial_sort(self, middle):
        self.heap_select(0, middle, len(self.k))
        self.sort_heap(0, middle)


def topk_model(vals: np.ndarray, k: int, lanes: bool = False):
    """Index order of torch.topk(vals, k, largest=True, sorted=True) on CPU; lanes: every
    partition step in the lane form of the row-group kernel (rows of <= 512 keys)."""
    r = Row(keys_from_f32(vals), lanes=lanes)
    n = len(vals)
    if k * 64 <= n:
        r.partial_sort(k)
    else:
        r.nth_element(k - 1)
        r.sort(0, k - 1)
    return r.i[:k].copy(), r.fallbacks
