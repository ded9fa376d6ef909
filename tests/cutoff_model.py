"""CPU model of the HIP cutoff (effort_amd/csrc/cutoff_device.h: block_find_cutoff) that also says WHICH BRANCHES it took.
TEST INFRASTRUCTURE: numpy only (no torch, no project code).

``model_cutoff(v, probes_u16, q, cap=4096, window=False)`` restates block_find_cutoff's control flow in numpy f32 arithmetic -- the
ballot rounds for value ranges wider than the table, the table of ``cap`` = kCutoffBinsPerThread * NT cells (NT = 128, 256, 512, 1024
threads: 1024, 2048, 4096, 8192 cells), the fixed window plain grids count into before the value range is known (``window=True``: the
PREZERO instantiations), the five order statistics one wave reads out of the histogram, the rounds run 16 at a time, the closed-form
tail -- asserts every shortcut against the count it stands for, and returns the cutoff with a path record:

  passes         ballot rounds before the table
  after_passes   "exit" (the loop ended inside a ballot round), "adjacent" (bounds in adjacent cells: no table), "table"
  lo_set, hi_set, above     at the table: whether a ballot round set the lower / the upper bound, and the values beyond the top cell
  table          "window" | "rebuilt-low" (smallest nonzero below the window) | "rebuilt-high" (largest beyond its last cell) |
                 "rebuilt-after-passes" | "range" (window=False); None without a table
  guards         per T(m-2) .. T(m+2): the guards that decided it, of "k<=0", "k>4096", "allGE<k", "sgAll>=64" (the last one only
                 where k > 0: every count, the one above the table's last cell included, reaches k)
  table_rounds, table_blocks    rounds spent in the table phase, and blocks of K_BLK rounds they took
  exit           "count-equal" | "bounds-1e-5" | "counts-within-3" | "hundred-rounds" | "fixed-point" (the reference's exits, the
                 first that holds in the reference's order) | "tail-closed-form" (X >= 128, at most 60 rounds spent) | "tail-loop"
  tail_late      a tail entered after more than 60 rounds
  rounds         the reference's loop counter at the end (the closed-form tail counts 19)
"""
import numpy as np

F = np.float32
NO_LO, NO_HI = 0xFFFF0000, 0xFFF00000
K_BLK = 16
WINDOW_BASE = (127 - 10) << 7          # kCutoffWindowBase: the cell of 2^-10
CAPS = (1024, 2048, 4096, 8192)        # kCutoffBinsPerThread x 128 / 256 / 512 / 1024 threads
GUARDS = ("k<=0", "k>4096", "allGE<k", "sgAll>=64")
EXITS = ("count-equal", "bounds-1e-5", "counts-within-3", "hundred-rounds", "fixed-point", "tail-closed-form", "tail-loop")


def _bf16(x):
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return r.astype(np.uint32).view(np.float32)


def cells(v, probes_u16):
    """The 4096 values bf16(|(1e5 * v[j]) * bf16(probe[j])|) as their 16-bit patterns: the model's ``vp``."""
    pr = _bf16(np.asarray(probes_u16).view(np.float16).astype(np.float32))
    with np.errstate(over="ignore", under="ignore"):
        t = (F(100000.0) * np.asarray(v).astype(np.float32)).astype(np.float32)
        vals = _bf16(np.abs((t * pr).astype(np.float32)))
    return (vals.view(np.uint32) >> 16).astype(np.int64)


def frompat(p):
    return np.asarray(np.uint32(int(p) << 16)).view(np.float32)[()]


def _pat(f):
    return int(np.asarray(F(f)).view(np.uint32)) >> 16


def _bits(f):
    return int(np.asarray(F(f)).view(np.uint32))


def _cell_edge_tail(nb, lo, hi, X, loops):
    """bisect_to_cell_edge: the loop form, and -- where the device takes it -- the closed form asserted against it.
    Returns (cutoff, rounds, label)."""
    closed = bool(X >= F(128.0)) and loops <= 60
    start = loops
    while True:
        loops += 1
        if nb >= X:
            hi = nb
        else:
            lo = nb
        prev = nb
        nb = F((hi + lo) / F(2))
        if F(hi - lo) < F(0.00001) or loops > 100 or nb == prev:
            break
    if closed:
        assert _bits(nb) == _bits(X) and loops - start <= 19, (nb, X, loops - start)
        return F(X), start + 19, "tail-closed-form"
    return nb, loops, "tail-loop"


def _device_order_statistic(hist, base, above, k, cap):
    """T(k) as wave 0 computes it from the histogram (cutoff_device.h, "one wave turns the histogram into the five order
    statistics"): lane L sums its kSeg = cap / 64 consecutive cells; a suffix scan over the lanes gives the count above each lane's
    last cell; whole lanes whose last cell still reaches k count in full; the boundary lane's cells are read kSub = ceil(kSeg / 64) per
    lane and scanned the same way, the last batch first.  Returns (T(k), the guards that decided it)."""
    seg = cap // 64
    sub = (seg + 63) // 64
    lanes = hist.reshape(64, seg).sum(axis=1)
    total = int(lanes.sum())
    c1 = above + total - np.cumsum(lanes)                          # count(last cell of lane L) = everything in later lanes, + above
    allGE = above + total
    sgAll = int((c1 >= k).sum())                                   # (the counts fall with the lane: a prefix)
    assert all(c1[i] >= c1[i + 1] for i in range(63))
    sg = min(sgAll, 63)
    lane = np.arange(64)
    later = int(c1[sg])
    n = sg * seg
    cnt = [None] * sub
    for u in range(sub - 1, -1, -1):                               # count(cell) = everything in later cells
        idx = u * 64 + lane
        x = np.where(idx < seg, hist[sg * seg + np.minimum(idx, seg - 1)], 0)
        p2 = np.cumsum(x)
        t2 = int(p2[63])
        cnt[u] = later + t2 - p2
        later += t2
    for u in range(sub):
        n += int(((u * 64 + lane < seg) & (cnt[u] >= k)).sum())
    hit = []
    if k <= 0:
        hit.append("k<=0")
    elif sgAll >= 64:
        hit.append("sgAll>=64")
    if k <= 0 or sgAll >= 64:
        return 0xFFFFFFFF, hit
    if k > 4096:
        hit.append("k>4096")
    if allGE < k:
        hit.append("allGE<k")
    if k > 4096 or allGE < k:
        return 0, hit
    return base + n, hit


def _block_rounds(nb, lo, hi, pLo, pHi, catLo, catHi, loops, T):
    """cutoff_device.h, "THE ROUNDS, kBlk AT A TIME": a block runs the bare recurrence of the bounds for K_BLK rounds (every lane
    the same), round r leaving its midpoint in lane r; lane r then reconstructs round r -- the bounds after it are the latest
    midpoints at or before r that went each way -- and evaluates the reference's exits; the first lane that stops hands over.
    Returns (fin, nb, lo, hi, pLo, pHi, loops, blocks) where the loop stops (fin: an exit of the reference; else adjacent cells)."""
    tM2, tM1, tM, tP1, tP2 = T
    tMs = 0xFFFFFFFF if tM >= 0x10000 else tM << 16
    if pHi == pLo + 1:
        return (False, nb, lo, hi, pLo, pHi, loops, 0)
    blocks = 0
    while True:
        blocks += 1
        a, l, h, rec = nb, lo, hi, []
        for r in range(K_BLK):                                   # the recurrence: runs on past the stop, harmlessly
            rec.append(a)
            below = _bits(a) >= tMs
            h, l = (a, l) if below else (h, a)
            a = F((h + l) / F(2))
        went = [_bits(x) >= tMs for x in rec]
        for r in range(K_BLK):                                   # "lane r"
            hs = [j for j in range(r + 1) if went[j]]
            ls = [j for j in range(r + 1) if not went[j]]
            hr, lr = (rec[hs[-1]] if hs else hi), (rec[ls[-1]] if ls else lo)
            pHr, pLr = (_bits(hr) >> 16 if hs else pHi), (_bits(lr) >> 16 if ls else pLo)
            cHr = int(pHr < tM1) + int(pHr < tM2) if hs else catHi
            cLr = int(pLr < tP1) + int(pLr < tP2) if ls else catLo
            p = _bits(rec[r]) >> 16
            nbr = F((hr + lr) / F(2))
            finr = (tP1 <= p < tM) or bool(F(hr - lr) < F(0.00001)) or cHr > cLr or loops + r + 1 > 100 or bool(nbr == rec[r])
            if finr or pHr == pLr + 1 or r == K_BLK - 1:
                state = (nbr, lr, hr, pLr, pHr, cLr, cHr)
                stopped = finr or pHr == pLr + 1
                break
        nb, lo, hi, pLo, pHi, catLo, catHi = state
        loops += r + 1
        if stopped:
            return (bool(finr), nb, lo, hi, pLo, pHi, loops, blocks)


def _exit_label(cntEq, bounds, within3, loops, fixed):
    """The reference's exits in the reference's order (:227-229, :236, and the fixed point)."""
    if cntEq:
        return "count-equal"
    if bounds:
        return "bounds-1e-5"
    if within3:
        return "counts-within-3"
    if loops > 100:
        return "hundred-rounds"
    assert fixed
    return "fixed-point"


def model_cutoff(v, probes_u16, q, cap=4096, window=False):
    """(cutoff, path record) of block_find_cutoff<cap / 8, PREZERO = window> on the 4096 inputs ``v`` and probes, quantile ``q``."""
    assert cap in CAPS
    vp = cells(v, probes_u16)
    effort = 4096 - q
    pmin, pmax = int(vp.min()), int(vp.max())
    nz = vp[vp > 0]
    pminNZ = min(int(nz.min()) if nz.size else 0xFFFF, pmax)
    lo, hi = F(min(frompat(pmin), F(1000.0))), F(frompat(pmax))
    nb = F((lo + hi) / F(2))
    loops, minC, maxC, pLo, pHi, done = 0, 4096, 0, NO_LO, NO_HI, False
    CA = lambda p: int((vp > p).sum())                                               # noqa: E731
    path = {"cap": cap, "window": bool(window), "passes": 0, "after_passes": None, "lo_set": False, "hi_set": False, "above": 0, "table": None,
            "guards": [[] for _ in range(5)], "table_rounds": 0, "table_blocks": 0, "exit": None, "tail_late": False, "rounds": 0}

    def rnd(cnt):                                                                    # `round` of the device code
        nonlocal loops, lo, hi, nb, minC, maxC, pLo, pHi
        loops += 1
        p = _pat(nb)
        if cnt < effort:
            hi, maxC, pHi = nb, cnt, p
        else:
            lo, minC, pLo = nb, cnt, p
        prev = nb
        nb = F((hi + lo) / F(2))
        bounds, within3 = bool(F(hi - lo) < F(0.00001)), abs(maxC - minC) < 3
        if cnt == effort or bounds or within3 or loops > 100 or nb == prev:
            path["exit"] = _exit_label(cnt == effort, bounds, within3, loops, nb == prev)
            return True
        return False
    low = lambda: max(pLo, pminNZ) if pLo != NO_LO else pminNZ                       # noqa: E731
    top = lambda: pHi if pHi != NO_HI else pmax                                      # noqa: E731
    while not done and pHi != pLo + 1 and top() - low() + 1 > cap:
        done = rnd(CA(_pat(nb)))
        path["passes"] += 1

    def finish(cutoff):
        path["rounds"] = loops
        return cutoff, path

    def tail():
        nonlocal loops
        path["tail_late"] = loops > 60
        c, loops, path["exit"] = _cell_edge_tail(nb, lo, hi, frompat(pHi), loops)
        return finish(c)
    if done:
        path["after_passes"] = "exit"
        return finish(nb)
    if pHi == pLo + 1:
        path["after_passes"] = "adjacent"
        return tail()
    path["after_passes"] = "table"
    base, tp = low(), top()
    above = maxC if pHi != NO_HI else 0
    path["lo_set"], path["hi_set"], path["above"] = pLo != NO_LO, pHi != NO_HI, above
    allGE = int((vp >= base).sum())

    def count_above(p):                                                              # the table lookup
        if p < base:
            return allGE
        if p > tp:
            return above
        return int((vp > p).sum())
    # tbl[c] = count_above(base + c) for the cells up to the top one, `above` beyond it (the plain count, all cells at once)
    gt = 4096 - np.cumsum(np.bincount(vp, minlength=0x10000 + cap))                  # gt[p] = #{values with pattern > p}
    tbl = np.where(base + np.arange(cap) <= tp, gt[base:base + cap], above)
    assert tbl[0] == count_above(base) and tbl[min(tp - base, cap - 1)] == count_above(min(tp, base + cap - 1))
    assert (tbl[:-1] >= tbl[1:]).all()

    def first_cell_below(k):                                                         # T(k): count(p) >= k  <=>  p < T(k)
        if k <= 0:
            return 0xFFFFFFFF
        if k > 4096 or allGE < k:
            return 0
        n = int((tbl >= k).sum())
        return 0xFFFFFFFF if n == cap else base + n
    m = effort
    T = tuple(first_cell_below(m + d) for d in (-2, -1, 0, 1, 2))
    tM2, tM1, tM, tP1, tP2 = T
    # the device finds the same five cells from the HISTOGRAM, one wave, two levels -- of the cells [base, top], rebuilt once the range
    # is known, or (PREZERO) of the fixed window it counted into before that, used iff no ballot pass ran and every nonzero value lies inside
    # (both forms are checked whatever ``window`` says; the path record follows the form the instantiation uses)
    hist = np.bincount((vp[(vp >= base) & (vp <= tp)] - base).astype(np.int64), minlength=cap)
    assert hist.size == cap                                                          # (the cells [base, top] fit the table)
    stats = [_device_order_statistic(hist, base, above, m + d, cap) for d in (-2, -1, 0, 1, 2)]
    assert tuple(s[0] for s in stats) == T, (stats, T)
    in_window = path["passes"] == 0 and pminNZ >= WINDOW_BASE and pmax - WINDOW_BASE < cap
    if in_window:
        win = np.bincount((vp[vp >= WINDOW_BASE] - WINDOW_BASE).astype(np.int64), minlength=cap)
        assert win.size == cap and above == 0
        wstats = [_device_order_statistic(win, WINDOW_BASE, 0, m + d, cap) for d in (-2, -1, 0, 1, 2)]
        assert tuple(s[0] for s in wstats) == T, (wstats, T)
    if not window:
        path["table"] = "range"
    elif in_window:
        path["table"], stats = "window", wstats
    elif path["passes"]:
        path["table"] = "rebuilt-after-passes"
    else:
        path["table"] = "rebuilt-low" if pminNZ < WINDOW_BASE else "rebuilt-high"
    path["guards"] = [s[1] for s in stats]
    # count(hi) as "how many of m-1, m-2 it reaches", count(lo) as "how many of m+1, m+2": |maxCount - minCount| < 3 <=> catHi > catLo
    catHi = int(pHi < tM1) + int(pHi < tM2) if pHi != NO_HI else int(maxC >= m - 1) + int(maxC >= m - 2)
    catLo = int(pLo < tP1) + int(pLo < tP2) if pLo != NO_LO else int(minC >= m + 1) + int(minC >= m + 2)
    loops0 = loops
    blk = _block_rounds(nb, lo, hi, pLo, pHi, catLo, catHi, loops, T)                # the device's block form, from the same state
    fin = False
    while not fin and pHi != pLo + 1:
        p = _pat(nb)
        cnt = count_above(p)                                                         # (the model checks every shortcut against the count)
        below = p >= tM
        assert below == (cnt < m)
        loops += 1
        if below:
            hi, pHi, catHi = nb, p, int(p < tM1) + int(p < tM2)
        else:
            lo, pLo, catLo = nb, p, int(p < tP1) + int(p < tP2)
        prev = nb
        nb = F((hi + lo) / F(2))
        cntEq = tP1 <= p < tM
        dLt3 = catHi > catLo
        mx = count_above(pHi) if pHi != NO_HI else maxC
        mn = count_above(pLo) if pLo != NO_LO else minC
        assert cntEq == (cnt == m) and dLt3 == (abs(mx - mn) < 3), (cntEq, cnt, m, dLt3, mx, mn)
        bounds = bool(F(hi - lo) < F(0.00001))
        fin = cntEq or bounds or dLt3 or loops > 100 or bool(nb == prev)
        if fin:
            path["exit"] = _exit_label(cntEq, bounds, dLt3, loops, bool(nb == prev))
    # the block form stops in the same round with the same state, bit for bit
    same = lambda x, y: _bits(x) == _bits(y)                                         # noqa: E731
    assert blk[0] == fin and same(blk[1], nb) and same(blk[2], lo) and same(blk[3], hi) and blk[4:7] == (pLo, pHi, loops), (blk, fin, nb, lo, hi, pLo, pHi, loops)
    path["table_rounds"], path["table_blocks"] = loops - loops0, blk[7]
    if fin:
        return finish(nb)
    return tail()
