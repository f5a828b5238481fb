"""TEST INFRASTRUCTURE: a float64 restatement of the nucleus (top-p) sampler, independent of the product code (plain NumPy, no import of the
package), against which the device sampler (csrc/emo_nucleus.h) is held at its edges.  Written from the reference's
stage2_accompaniment/inference.py:71-100 (temperature() + nucleus()) and from the contract the header states:

  probabilities   softmax(logits / temp);
  order           descending probability, ties by ASCENDING INDEX.  That is this project's rule.  The reference's order among exact ties is
                  whatever NumPy's unstable argsort produces (on the golden fixtures neither ascending nor descending index);
  cut             with cum = cumsum(sorted probabilities): no entry exceeds top_p -> the top min(V, 3); only the last entry does (the reference
                  raises IndexError) -> all V; otherwise the first crossing and the token after it (the reference's `np.where(after)[0][1]`);
  draw            searchsorted(cdf of the renormalised candidates, u, side='right'), clamped to the last candidate.

The sampler works in fp32 (and the reference in another fp32 order: no max subtraction, a pairwise and then a sequential sum, two divides), so its
cumulative sum differs from the float64 one in the last bits, and where that sum lands within rounding of top_p the cut may legitimately move by one
token.  The bounds that separate this from an error are DERIVED, not tuned:

  m = (V + 16) 2^-24   (margin)   worst-case absolute error of a sequential fp32 sum of V non-negative terms whose total is <= 1 (one rounding of at
                       most 2^-24 per add), plus a few ulp per term for expf and the normalisation.  cut_bracket() evaluates the cut rule at
                       top_p - m and top_p + m; a row where the two differ is a KNIFE-EDGE row and only its cut length and containment are checked.
  DELTA = 32 2^-24     a few ulp of relative error per probability carried into a ratio of sums, plus the rounding of u itself: how far a CDF
                       boundary of the sampler may lie from the float64 one.
  TIE_REL = 8 2^-24    two float64 probabilities closer than this (relative) may collide in fp32, where the sampler then orders them by index:
                       such tokens count as the same rank.

A sampler outside these bounds is a finding; the bounds are not to be widened to make it pass."""
import numpy as np

ULP = 2.0 ** -24
DELTA = 32 * ULP
TIE_REL = 8 * ULP
U_MAX = np.nextafter(np.float32(1), np.float32(0))          # the largest float32 below 1

# (V, scale, temp, top_p): rows are standard_normal(V) * scale, cast to float32 (family_rows)
FAMILIES = ((327, 4.0, 1.1, 0.9), (327, 1.0, 1.2, 0.97), (200, 2.0, 1.2, 0.9), (40, 2.0, 1.1, 0.99), (370, 3.0, 1.0, 0.5), (1000, 4.0, 1.2, 0.9),
            (1024, 4.0, 1.0, 0.97), (1017, 6.0, 1.1, 0.9), (7, 1.0, 1.2, 0.9), (65, 2.0, 5.0, 0.9), (513, 4.0, 1.0, 0.3))


def family_rows(rng, V, scale, rows):
    return (rng.standard_normal((rows, V)) * scale).astype(np.float32)


def margin(V):
    return (V + 16) * ULP


def probs64(logits_f32, temp):
    """float64 softmax of logits / temp, the maximum subtracted; -inf logits give exactly 0.  temp is the float32 the sampler is handed."""
    x = np.asarray(logits_f32, dtype=np.float32).astype(np.float64) / np.float64(np.float32(temp))
    e = np.exp(x - x.max())
    return e / e.sum()


def order(probs):
    """Token ids by descending probability, ties by ascending index."""
    return np.lexsort((np.arange(len(probs)), -np.asarray(probs)))


def cut_count(cum, top_p, V):
    """The three-branch rule on the inclusive cumulative sum of the sorted probabilities -> number of candidates."""
    i1 = int(np.count_nonzero(cum <= top_p))               # cum is non-decreasing: the first crossing, and i1 + 1 the second
    if i1 >= V:
        return min(V, 3)                                   # no crossing
    if i1 + 1 >= V:
        return V                                           # single crossing (reference: IndexError)
    return i1 + 1


def cut_bracket(probs64_sorted, top_p, V):
    """(n_lo, n_hi): the candidate counts of the rule at top_p - m and top_p + m."""
    cum = np.cumsum(probs64_sorted)
    m = margin(V)
    return cut_count(cum, top_p - m, V), cut_count(cum, top_p + m, V)


def expected_pick(cands, probs, u):
    w = np.asarray(probs, dtype=np.float64)[cands]
    cdf = np.cumsum(w) / w.sum()
    return int(cands[min(int(np.searchsorted(cdf, np.float64(u), side='right')), len(cands) - 1)])


def same_rank(pa, pb):
    return abs(pa - pb) <= TIE_REL * max(pa, pb)


class Row:
    """Everything the checks need of one (logits, temp, top_p): probabilities, order, bracket, and the probes of its CDF."""

    def __init__(self, logits, temp, top_p, n_fixed=None):
        self.logits = np.ascontiguousarray(logits, dtype=np.float32)
        self.temp, self.top_p, self.V = float(temp), float(top_p), len(self.logits)
        self.probs = probs64(self.logits, temp)
        self.order = order(self.probs)
        self.ps = self.probs[self.order]
        self.nnz = int(np.count_nonzero(self.ps))          # ranks count only tokens of non-zero probability (zeros sort last)
        self.pos = np.empty(self.V, dtype=np.int64)
        self.pos[self.order] = np.arange(self.V)
        self.n_lo, self.n_hi = cut_bracket(self.ps, top_p, self.V) if n_fixed is None else (n_fixed, n_fixed)
        self.knife = self.n_lo != self.n_hi
        # candidates that can be drawn: a zero-probability token inside the cut (no-crossing top 3, single-crossing all V) has an empty interval
        self.k_lo, self.k_hi = (min(n, self.nnz) for n in (min(self.n_lo, self.n_hi), max(self.n_lo, self.n_hi)))
        if not self.knife:
            self.cands = self.order[:self.k_hi]
            w = self.probs[self.cands]
            self.cdf = np.cumsum(w) / w.sum()              # cdf[i] = upper boundary b_i of candidate i's interval [b_{i-1}, b_i)
            self.width = np.diff(self.cdf, prepend=0.0)

    def rank_span(self, tok):
        """[lo, hi]: the sorted positions that count as the rank of token `tok` (TIE_REL); None for a zero-probability token."""
        p = self.probs[tok]
        if p == 0.0:
            return None
        asc = self.ps[:self.nnz][::-1]
        lo = self.nnz - int(np.searchsorted(asc, p / (1 - TIE_REL), side='right'))
        hi = self.nnz - 1 - int(np.searchsorted(asc, p * (1 - TIE_REL), side='left'))
        return lo, hi

    def narrow(self):
        """Candidates whose CDF interval is too narrow (<= 2 DELTA) for the midpoint probe."""
        return int(np.count_nonzero(self.width <= 2 * DELTA))

    def probes(self):
        """(u float32 [R], expected candidate position int [R], -1 where only cut length / containment apply).  Always: u = 0 (rank 0) and U_MAX
        (the last candidate).  Rows that are not knife-edge: the float32 midpoint of every interval wider than 2 DELTA, and b_i -+ 2 DELTA wherever
        both neighbouring intervals are wider than 4 DELTA."""
        u, e = [np.float32(0), U_MAX], [0, -1]
        if not self.knife:
            n, b, w = len(self.cands), self.cdf, self.width
            for i in range(n):
                if w[i] > 2 * DELTA:
                    u.append(np.float32(b[i] - 0.5 * w[i]))
                    e.append(i)
            for i in range(n - 1):
                if w[i] > 4 * DELTA and w[i + 1] > 4 * DELTA:
                    u += [np.float32(b[i] - 2 * DELTA), np.float32(b[i] + 2 * DELTA)]
                    e += [i, i + 1]
        else:                                              # containment only: a plain sweep
            u += list(np.linspace(0, 1, 64, endpoint=False, dtype=np.float32))
            e += [-1] * 64
        return np.array(u, dtype=np.float32), np.array(e, dtype=np.int64)

    def check(self, u, got):
        """Cut length, containment and draw of the picks `got` at the probes `u` of probes() (any sampler: ids as integers)."""
        _, exp = self.probes()
        assert len(got) == len(exp)
        spans = {}
        for r, (t, ei) in enumerate(zip(got, exp)):
            t = int(t)
            assert 0 <= t < self.V, ('id out of range', r, t)
            sp = spans.get(t)
            if sp is None:
                sp = spans[t] = self.rank_span(t)
            assert sp is not None, ('a token of probability 0 was drawn', r, t, float(u[r]))
            assert sp[0] < self.k_hi, ('pick outside the candidate set', r, t, sp, self.k_hi, float(u[r]))              # containment
            if r == 0:
                assert sp[0] == 0, ('u = 0 must give the most likely token', t, sp)
            elif r == 1:
                assert sp[1] >= self.k_lo - 1, ('cut too short: last candidate', t, sp, (self.k_lo, self.k_hi))          # cut length
            elif ei >= 0:
                c = int(self.cands[ei])
                assert t == c or same_rank(self.probs[t], self.probs[c]), ('draw', r, float(u[r]), 'got', t, 'expected', c, 'interval', int(ei))
        return {int(t) for t in got}
