"""numpy restatement of roma_op_sample_matches (roma_amd.sample_matches, csrc/sample_batched.hip): RegressionMatcher.sample
(romatch/models/matcher.py:598-629) of ONE pair from its seed, with the race keys and the density in float64.

The device's definition, term for term (include/roma_hip.h):
  * u of row i from two rounds of the splitmix64 finaliser on (seed, i), 23 bits + 0.5 over 2^23 - integers and u are exactly the
    device's; key = min(-log(u) / w, 3e38), +inf for w <= 0 - the device's in f32 with __logf, so equal to ~1e-6 relative;
  * a draw = the k smallest keys in ascending (key, index) order: draw order, ties to the lowest index, the +inf filler entries
    of a pair with fewer than k positive weights included;
  * p = 1 / (density + 1), 1e-7 where density < 10, 0 for a drawn row whose (thresholded) certainty is not positive;
  * the second draw runs over j = 0 .. k - 1 on seed ^ SECOND_DRAW_SEED.
`density=` replaces this file's own density (f64 over the fp16-rounded coordinates) by the caller's, so that the second draw can
be driven from the device's."""
import numpy as np

SECOND_DRAW_SEED = 0x5851f42d4c957f2d  # csrc/sample_batched.hip SAMPLE_SECOND_DRAW_SEED
KEY_MAX = 3.0e38
MASK = (1 << 64) - 1


def mix64(z):
    """splitmix64 finaliser on a uint64 array (csrc/sampling.h)"""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def uniforms(seed, n):
    """u of rows 0 .. n - 1 (float64; exact: 23 random bits + 0.5, over 2^23)"""
    seed = np.uint64(int(seed) & MASK)
    with np.errstate(over="ignore"):
        r = mix64(mix64(seed + np.uint64(0x9e3779b97f4a7c15) * (np.arange(n, dtype=np.uint64) + np.uint64(1))) ^ seed)
    return ((r >> np.uint64(41)).astype(np.float64) + 0.5) / 8388608.0


def race_keys(weights, seed):
    """float64 keys of the exponential race"""
    w = np.asarray(weights, dtype=np.float64)
    key = np.full(w.shape, np.inf)
    pos = w > 0
    key[pos] = np.minimum(-np.log(uniforms(seed, len(w))[pos]) / w[pos], KEY_MAX)
    return key


def draw(weights, k, seed):
    """(indices of the k smallest keys in ascending (key, index) order, all keys)"""
    key = race_keys(weights, seed)
    order = np.lexsort((np.arange(len(key)), key))
    return order[:k], key


def density_f64(x, std=0.1):
    """Gaussian kernel density of the rows of x [k, 4] among themselves, coordinates rounded to fp16, float64 sum"""
    h = np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float64)
    out = np.empty(len(h))
    for s in range(0, len(h), 1024):
        d2 = ((h[s:s + 1024, None, :] - h[None, :, :]) ** 2).sum(-1)
        out[s:s + 1024] = np.exp(-d2 / (2.0 * std * std)).sum(-1)
    return out


def balance_weights(density, certainty):
    """p of the second draw, float32 like the device's: 1 / (density + 1), 1e-7 where density < 10, 0 for a filler row"""
    d = np.asarray(density, dtype=np.float32)
    p = (np.float32(1) / (d + np.float32(1))).astype(np.float32)
    p[d < 10] = np.float32(1e-7)
    p[~(np.asarray(certainty) > 0)] = 0
    return p


def sample(matches, certainty, num=10000, sample_mode="threshold_balanced", sample_thresh=0.05, seed=0, density=None):
    """One pair: matches [n, 4], certainty [n] (any leading shape is flattened).  Returns a dict with
    matches [m, 4], certainty [m], idx [m] (into the n rows), count (leading real rows), first_idx [k], keys1 [n] (float64),
    and in the balanced modes density [k], p [k] (float32), keys2 [k] (float64), second [m] (indices into the k rows)."""
    x = np.asarray(matches, dtype=np.float32).reshape(-1, 4)
    c = np.asarray(certainty, dtype=np.float32).reshape(-1).copy()
    if "threshold" in sample_mode:
        c[c > np.float32(sample_thresh)] = 1
    n = len(c)
    balanced = "balanced" in sample_mode
    k = min(4 * num if balanced else num, n)
    m = min(num, k)
    first, keys1 = draw(c, k, seed)
    out = dict(first_idx=first, keys1=keys1, count=min(m, int((c > 0).sum())))
    if not balanced:
        out.update(idx=first, matches=x[first], certainty=c[first])
        return out
    gx, gc = x[first], c[first]
    dens = density_f64(gx) if density is None else np.asarray(density)
    p = balance_weights(dens, gc)
    second, keys2 = draw(p, m, int(seed) ^ SECOND_DRAW_SEED)
    out.update(density=dens, p=p, keys2=keys2, second=second, idx=first[second], matches=gx[second], certainty=gc[second])
    return out
