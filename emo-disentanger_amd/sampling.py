"""Host-side token sampling with the reference's observable behaviour, written from its specification:

temperature  (stage2 inference.py:71-83, stage1 inference_utils.py:14-24)
    p = exp(l / t) / sum(exp(l / t)) evaluated in the logits' own dtype (float32 from the model); when that produces a NaN
    (overflow) the computation is repeated in 128-bit floats and returned as float64.  Optional `inadmissibles` get -inf first.
nucleus      (inference.py:86-100, inference_utils.py:27-41)
    renormalise by the left-to-right sum of the array (same dtype), sort descending, running sum; the candidate set ends ONE
    position after the first prefix whose mass exceeds p (the reference indexes the SECOND crossing: the crossing token is kept,
    and a distribution with exactly one crossing raises IndexError — tests/golden/sampling.json pins both); if no prefix exceeds
    p the top three are taken; the candidates are renormalised in float64 and one is drawn with NumPy's global RNG (or `rng`).

Bit-exactness notes: np.cumsum accumulates strictly left to right in the array's dtype, which is what Python's built-in sum()
over a NumPy array does, while np.sum() is pairwise; ties in the ranking come from np.argsort's default kind, like the reference."""
import numpy as np


def _sequential_total(a):
    return np.cumsum(a)[-1]


def temperature(logits, temperature, inadmissibles=None, longdouble_softmax=False):
    """longdouble_softmax: stage 1 finishes the overflow path with a max-shifted softmax (scipy.special.softmax there)."""
    if inadmissibles is not None:
        logits[inadmissibles] -= np.inf
    with np.errstate(over='ignore', invalid='ignore'):
        e = np.exp(logits / temperature)
        probs = e / np.sum(e)
    if np.isnan(probs).any():
        print('overflow detected, use 128-bit')
        z = logits.astype(np.float128) / temperature
        if longdouble_softmax:
            z = z - z.max()
        e = np.exp(z)
        probs = (e / np.sum(e)).astype(float)
        if longdouble_softmax:
            assert not np.isnan(probs).any()
    return probs


def soft_cut_count(sorted_probs, last, top_k=0, min_p=0.0):
    """The two cuts behind top-p, as the device draw makes them (csrc/emo_nucleus.h: emo_nucleus_pick) -> the candidate count
    min(last, k-cut, n_m).  sorted_probs: the probabilities in rank order (descending; among equal ones the caller's tie rule: ascending index
    on the device, so a tie group that straddles top_k keeps its lowest indices); last: the count top-p gives, with all its edge rules.
    top_k: an integer, <= 0 off, k = 1 greedy, k >= V no cut.  min_p: <= 0 off; n_m = #{i : sp[i] >= m * sp[0]} in the array's own dtype (one
    rounded float32 multiply on float32 probabilities, as on the device), at least 1, also for m > 1."""
    sp = np.asarray(sorted_probs)
    count = min(int(last), len(sp))
    if top_k > 0:
        count = min(count, int(top_k))
    if min_p > 0:
        thr = sp.dtype.type(min_p) * sp[0] if sp.dtype.kind == 'f' else float(min_p) * sp[0]
        count = min(count, max(1, int(np.count_nonzero(sp >= thr))))
    return count


def biased(logits, bias):
    """The row the draw reads under an additive bias: float32 `l + b`, one rounded add per token (-inf entries act as a ban); None: the row."""
    return logits if bias is None else np.asarray(logits, np.float32) + np.asarray(bias, np.float32)


def nucleus_candidates(probs, p, top_k=0, min_p=0.0):
    """-> (candidate ids in rank order, their float64 weights).  `probs` is renormalised IN PLACE like the reference does.  top_k / min_p: the
    two cuts of soft_cut_count behind the reference's rule (both off: the reference's candidates).  On the single-crossing edge the reference's
    IndexError is raised BEFORE any cut, as without the controls, while the device keeps all V there and then cuts: on that one edge this
    function and the device do not agree (pick_at restates the device)."""
    probs /= _sequential_total(probs)
    order = np.argsort(probs)[::-1]
    srt = np.sort(probs)[::-1]
    mass = np.cumsum(srt)
    crossings = np.flatnonzero(mass > p)
    keep = crossings[1] if crossings.size else 3          # IndexError when there is exactly one crossing: reference behaviour (F12)
    if top_k > 0 or min_p > 0:
        keep = soft_cut_count(srt, keep, top_k, min_p)
    ids = order[:keep]
    w = probs[ids].astype(np.float64)
    return ids, w / _sequential_total(w)


def nucleus(probs, p, rng=None, top_k=0, min_p=0.0):
    ids, w = nucleus_candidates(probs, p, top_k, min_p)
    return (np.random if rng is None else rng).choice(ids, size=1, p=w)[0]


def pick_at(probs, top_p, u, top_k=0, min_p=0.0):
    """The candidate cut and the pick of the device draw from given probabilities (any float dtype; taken to float64 and renormalised) at the
    uniform u -> the token id: ranking descending with ties by ascending index, top-p's count (second crossing; single crossing: all, where
    nucleus_candidates raises the reference's IndexError; no crossing: top 3) cut by soft_cut_count, searchsorted(cumsum over the count, u * its
    total, 'right'), clamped.  A host loop whose sampler is this function on the device loop's uniforms makes the device's draws."""
    pr = np.asarray(probs, np.float64)
    pr = pr / pr.sum()
    V = len(pr)
    order = np.lexsort((np.arange(V), -pr))
    sp = pr[order]
    cum = np.cumsum(sp)
    i1 = int(np.count_nonzero(cum <= np.float64(np.float32(top_p))))
    last = min(V, 3) if i1 >= V else V if i1 + 1 >= V else i1 + 1
    last = soft_cut_count(sp, last, top_k, float(np.float32(min_p)))      # (the factor the device is handed: a float32)
    target = np.float64(np.float32(u)) * cum[last - 1]
    return int(order[min(int(np.searchsorted(cum[:last], target, side='right')), last - 1)])


def draw_at(logits, temp, top_p, u, bias=None, top_k=0, min_p=0.0, banned=None):
    """A float64 restatement of the device draw (csrc/emo_nucleus.h) at the uniform u, the soft controls included -> the token id.  The row is
    read as float32 `l + bias` with the banned ids at -inf, the probabilities are softmax(row / temp) in float64, and the id is pick_at's.  It
    agrees with the device wherever no float32 rounding decides (a prefix within rounding of top_p, a probability within rounding of the
    min_p threshold, a CDF boundary within rounding of u)."""
    row = np.array(biased(np.asarray(logits, np.float32), bias), np.float32)
    if banned is not None and len(banned):
        row[np.asarray(banned, np.int64)] = -np.inf
    x = row.astype(np.float64) / np.float64(np.float32(temp))
    e = np.exp(x - x.max())
    return pick_at(e / e.sum(), top_p, u, top_k, min_p)


def beat_position(event):
    """'Beat_7' -> 7"""
    return int(event.rsplit('_', 1)[1])


def event_name(idx2event, i):
    """The event of token id i in a dict or list vocabulary, None where it has none."""
    if isinstance(idx2event, dict):
        return idx2event.get(i)
    return idx2event[i] if i < len(idx2event) else None
