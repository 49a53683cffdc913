"""The reference the receive-window tests hold the library to (tests/test_rxwin_cpu.py through the CPU harness tests/rxwin_emul, tests/test_gpu_rxwin.py on the GPU),
written from the standards and from the contract in include/aesgcm.h "RECEIVE WINDOWS" -- never from the kernels' code:
  rfc4303_a21     the literal pseudo-code of RFC 4303 Appendix A2.1 in Th, Tl, W: which Seqh a receiver takes for Seql
  rfc3711_index   the literal pseudo-code of RFC 3711 Appendix A: which rollover counter v a receiver takes for SEQ
  lowest, srtp_v  the two recovery rules as the header states them (a definition each, on Python's unbounded integers)
  recover         a whole recover call: the refusals in the header's order, the rule, (num, hi) per packet
  Window          a SEQUENTIAL window -- the set of seen numbers and `next` -- that takes a call's authenticated packets in descending number order, RFC 4303 A2's
                  check-and-update one packet at a time; normalised() = the form of aesgcm_rxwin_set / _get
and the cases both test files run: call_sequence, sequences of commit calls placed around the windows' edges, with what the sequential window makes of each, and
ring_sequence, which adds the placements that a ring of more than one word needs (RING_MOVES; ring_move_kinds reads them off a sequence of states)."""
NONE = (1 << 64) - 1
WIRE, LOWEST, SRTP, EXPECT = 1, 2, 3, 4
FROM_END, CLEAR_TOP = 1, 2
NOAUTH, ACCEPT, OLD, REPLAY, REFUSED = range(5)


def rfc4303_a21(Th, Tl, W, Seql):
    """RFC 4303 Appendix A2.1, "Managing and Using the Anti-Replay Window": -> Seqh.  Arithmetic on Tl is modulo 2^32, as the 32-bit variables of the RFC are."""
    M = 1 << 32
    if Tl >= W - 1:                                 # Case A
        if Seql >= Tl - W + 1:
            Seqh = Th
        else:
            Seqh = Th + 1
    else:                                           # Case B
        if Seql >= (Tl - W + 1) % M:
            Seqh = Th - 1
        else:
            Seqh = Th
    return Seqh


def rfc3711_index(s_l, ROC, SEQ):
    """RFC 3711 Appendix A, "Pseudocode for Index Determination": -> v"""
    if s_l < 32768:
        if SEQ - s_l > 32768:
            v = (ROC - 1) % (1 << 32)
        else:
            v = ROC
    else:
        if s_l - 32768 > SEQ:
            v = (ROC + 1) % (1 << 32)
        else:
            v = ROC
    return v


def lowest(T, W, t, bits):
    """the smallest n >= B = max(T - W, 0) with n = t (mod 2^bits)"""
    B = max(T - W, 0)
    return B + (t - B) % (1 << bits)


def srtp_v(T, SEQ):
    """the header's AESGCM_RXWIN_SRTP: RFC 3711's rule without its wrap at either end -- nothing goes below ROC 0, and a v above 2^32 - 1 is for the caller to refuse"""
    if T == 0:
        return 0
    s_l, ROC = (T - 1) & 0xFFFF, (T - 1) >> 16
    if s_l < 32768:
        return max(ROC - 1, 0) if SEQ - s_l > 32768 else ROC
    return ROC + 1 if s_l - 32768 > SEQ else ROC


def recover(fmt, n_wins, W, nexts, wins, data, offs):
    """fmt = (rule, num_off, num_len, flags); nexts[w] = window w's next; packet p = data[offs[p]:offs[p + 1]] -> ([(num, hi)], lowest refused index or None)"""
    rule, num_off, num_len, flags = fmt
    out, bad = [], None
    for p, w in enumerate(wins):
        r = None
        if w < n_wins:
            T = nexts[w]
            if rule == EXPECT:
                if T != NONE:
                    r = (T, T >> 32)
            else:
                b, e = offs[p], offs[p + 1]
                n = e - b
                inside = e >= b and ((num_off <= n and num_len <= num_off) if flags & FROM_END else num_off + num_len <= n)
                if inside:
                    at = b + (n - num_off if flags & FROM_END else num_off)
                    t = int.from_bytes(data[at:at + num_len], "big")
                    if rule == WIRE:
                        if flags & CLEAR_TOP:
                            t &= ~(1 << (8 * num_len - 1))
                        if t < NONE:
                            r = (t, t >> 32)
                    elif rule == LOWEST:
                        full = lowest(T, W, t, 8 * num_len)
                        if full < NONE:
                            r = (full, (full >> (8 * num_len)) & 0xFFFFFFFF)
                    else:
                        v = srtp_v(T, t)
                        if v <= 0xFFFFFFFF:
                            r = (v << 16 | t, v)
        if r is None:
            r = (NONE, 0xFFFFFFFF)
            bad = p if bad is None else bad
        out.append(r)
    return out, bad


class Window:
    def __init__(self, W, next=0, seen=()):
        self.W, self.next, self.seen = W, next, set(seen)

    def one(self, num):
        """RFC 4303 A2's check-and-update for one authenticated packet"""
        if num >= self.next:                        # to the right of the window: it moves
            self.next = num + 1
            self.seen = {s for s in self.seen if s + self.W >= self.next}
            self.seen.add(num)
            return ACCEPT
        if num + self.W < self.next:
            return OLD
        if num in self.seen:
            return REPLAY
        self.seen.add(num)
        return ACCEPT

    def normalised(self):
        return self.next, sum(1 << (self.next - 1 - s) for s in self.seen)

    @classmethod
    def from_normalised(cls, W, next, seen):
        return cls(W, next, {next - 1 - i for i in range(W) if (seen >> i) & 1})


def commit(windows, wins, nums, auths):
    """one commit call over {w: Window}: -> why per packet.  Among the copies of one fresh (window, number) the FIRST in this order is the accepted one; which one the
    library accepts is unspecified, so callers compare such groups as multisets (same_verdicts)"""
    why = [None] * len(wins)
    S = []
    for p, (w, n, a) in enumerate(zip(wins, nums, auths)):
        if not a:
            why[p] = NOAUTH
        elif w not in windows or n == NONE:
            why[p] = REFUSED
        else:
            S.append(p)
    for p in sorted(S, key=lambda p: -nums[p]):     # descending number order: the window advances first
        why[p] = windows[wins[p]].one(nums[p])
    return why


def same_verdicts(wins, nums, got, want):
    """every packet's verdict as the reference's, the copies of one (window, number) compared as a multiset -- and never more than one of them accepted"""
    groups = {}
    for p, k in enumerate(zip(wins, nums)):
        groups.setdefault(k, []).append(p)
    for k, ps in groups.items():
        g, w = sorted(got[p] for p in ps), sorted(want[p] for p in ps)
        if g != w:
            return "window %d number %d: got %r, want %r" % (k[0], k[1], g, w)
        if k[1] != NONE and g.count(ACCEPT) > 1:
            return "window %d number %d accepted %d times" % (k[0], k[1], g.count(ACCEPT))
    return None


def call_sequence(rng, n_wins, W, n_pkts=None, sequence=10, first_next=0):
    """A sequence of commit calls (n_pkts packets each, or as many as the placements give) around each window's edges: numbers at next - W - 1, next - W, next - 1, next,
    next + W - 1, next + W, next + 5 W (a full clear), around 2^32, with next = 2^64 - 2; 2, 3 and 64 copies of one number; copies of numbers from the call before;
    forged packets far ahead; refused ones.  Window 0 starts at first_next, window 1 below 2^32, window 2 at 2^64 - 2, the others anywhere, each with random seen bits.
    -> (sets, calls): sets = [(window, next, seen)] for aesgcm_rxwin_set; calls = [(wins, nums, auths, why, [normalised state per window], lowest refused index or None)]"""
    state, sets = {}, []
    start = {0: first_next, 1: 2 ** 32 - W // 2, 2: 2 ** 64 - 2}
    for w in range(n_wins):
        nx = start.get(w, rng.randrange(2 ** 40))
        seen = rng.getrandbits(W) & ((1 << min(nx, W)) - 1)
        state[w] = Window.from_normalised(W, nx, seen)
        sets.append((w, nx, seen))
    calls, prev = [], []
    for k in range(sequence):
        pool = []
        for w in (range(n_wins) if n_wins <= 3 else rng.sample(range(n_wins), 4)):
            nx = state[w].next
            if k % 3 == 0:
                cand = [nx - W - 1, nx - W, nx - 1, nx, nx + W - 1, nx + W, nx + 5 * W, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1]
            elif k % 3 == 1:
                cand = [nx - rng.randrange(1, W), nx + rng.randrange(0, W // 2), nx + 1, nx - W // 2, nx + W - 1]
            else:
                cand = [nx + rng.randrange(0, 3 * W) for _ in range(6)] + [nx - 1]
            cand = [c for c in cand if 0 <= c <= 2 ** 64 - 2] or [nx - 1 if nx else 0]
            pool += [(w, c, 1) for c in cand]
            pool += [(w, rng.choice(cand), 1)] * (1, 2, 63)[(k + w) % 3]       # with the one above: 2, 3 and 64 copies of one number
            pool += [(w, min(nx + 100 * W, 2 ** 64 - 2), 0), (w, rng.choice(cand), 0)]      # forgeries, one far ahead
        pool += [p for p in prev if p[2] and p[0] < n_wins and p[1] != NONE][:5]  # copies of numbers of the call before
        pool += [(n_wins, 5, 1), (rng.randrange(n_wins), NONE, 1), (2 ** 32 - 1, NONE, 0)]
        rng.shuffle(pool)
        if n_pkts is not None:
            if len(pool) >= n_pkts:
                pool = [pool[(k + i) % len(pool)] for i in range(n_pkts)] if n_pkts < 8 else pool[:n_pkts]
            while len(pool) < n_pkts:                                          # the rest: reordered traffic around the windows, duplicates among it
                w = rng.randrange(n_wins)
                c = state[w].next + rng.randrange(-2 * W, 2 * W)
                pool.append((w, min(max(c, 0), 2 ** 64 - 2), 1 if rng.randrange(8) else 0))
        wins, nums, auths = zip(*pool)
        why = commit(state, wins, nums, auths)
        refused = [p for p in range(len(pool)) if why[p] == REFUSED]
        calls.append((wins, nums, auths, why, [state[w].normalised() for w in range(n_wins)], refused[0] if refused else None))
        prev = pool
    return sets, calls


# The partial clear of [next, M) on a ring of more than one word (W >= 128), as (next mod W, M - next): inside one word; ending exactly on a word boundary; over three
# or more words (at W = 128 the third is the first again); from the ring's last word into its first
RING_MOVES = {"inside": lambda W: (64 + 5, 20), "boundary": lambda W: (40, 24), "three": lambda W: (60, min(W - 8, 150)), "wrap": lambda W: (W - 10, 30)}


def ring_move_kinds(W, at, d):
    """which of RING_MOVES' kinds the clear of d positions from ring position `at` is (none for no move and for the full clear)"""
    kinds = set()
    if 0 < d < W:
        first, last = at >> 6, (at + d - 1) >> 6                                # the words of the unwrapped range
        if first == last:
            kinds.add("inside")
        if (at + d) % 64 == 0:
            kinds.add("boundary")
        if last - first >= 2:
            kinds.add("three")
        if at >> 6 == W // 64 - 1 and at + d > W:
            kinds.add("wrap")
    return kinds


def ring_sequence(rng, n_wins, W, n_pkts, first_next=0):
    """call_sequence's ten calls, then for each kind of RING_MOVES two more: one that brings a window's next to the kind's ring position (a full clear), one that moves it
    by the kind's distance over positions that the call before filled one and all, and up to one that it filled too and that must stay.  The window is the first that has room above it; the other windows carry reordered traffic meanwhile.
    Same return form as call_sequence; test_rxwin_cpu.py's recorded sequences come from call_sequence alone and do not change."""
    assert W >= 128 and n_pkts >= 200
    sets, calls = call_sequence(rng, n_wins, W, n_pkts=n_pkts, first_next=first_next)
    state = {w: Window.from_normalised(W, *calls[-1][4][w]) for w in range(n_wins)}
    r = next(w for w in range(n_wins) if state[w].next + 16 * W < 2 ** 63)

    def call(top, more=()):
        """n_pkts packets; window r's largest authenticated number is `top`, its others are `more` and numbers of the 2 W below"""
        pool = [(r, top, 1), (r, top, 1), (r, min(top + 50 * W, 2 ** 64 - 2), 0)] + [(r, x, 1) for x in more]
        while len(pool) < n_pkts:
            w = rng.randrange(n_wins)
            c = top - rng.randrange(0, 2 * W) if w == r else state[w].next + rng.randrange(-2 * W, 2 * W)
            pool.append((w, min(max(c, 0), 2 ** 64 - 2), 1 if rng.randrange(8) else 0))
        rng.shuffle(pool)
        wins, nums, auths = zip(*pool)
        why = commit(state, wins, nums, auths)
        assert REFUSED not in why
        calls.append((wins, nums, auths, why, [state[w].normalised() for w in range(n_wins)], None))

    for kind in ("inside", "boundary", "three", "wrap"):
        at, d = RING_MOVES[kind](W)
        nx = state[r].next
        top = nx + 2 * W + (at - nx) % W - 1                                     # next = at (mod W) behind this call
        low = top + 1 - W                                                        # ... and these numbers hold the positions the move clears, and the first behind them
        call(top, [low + j for j in range(d + 1)])
        assert state[r].next % W == at and low + d in state[r].seen
        call(state[r].next + d - 1)
        assert kind in ring_move_kinds(W, at, d) and low + d in state[r].seen and low + d - 1 not in state[r].seen
    return sets, calls
