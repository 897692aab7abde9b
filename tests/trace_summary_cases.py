"""Built traces for the trace-summary kernels (tests/test_gpu_trace_summary_kernels.py drives the kernels with them,
tests/test_trace_summary_reference.py the host classes): each case is named for the branch of csrc/posterior_kernel.hpp it
reaches and is built in every form it applies to -- one word per haplotype at ploidy 2, 4, 8; two words at ploidy 3, 10, 15; the
calling form (a word = an allele index) at ploidy 2, 4, 8.  States are tuples of Python ints, ascending
(tests/trace_summary_reference.py); every chain is prefixed with `burn` states that occur nowhere else."""
from itertools import combinations

from tests.trace_summary_reference import MASK64

BATCH_CAP = 512        # POST_CAP: the table of a batch launch (every form's LDS holds it; the GPU test asserts that)
LISTED_CAP = 70        # the table the full-table case gives the listed launch
POST_MAX_CHAINS = 32


class Form(object):
    """kind "w1" / "w2" / "call" at one ploidy: the symbols of a case -> haplotypes or alleles."""

    def __init__(self, kind, ploidy):
        self.kind, self.K = kind, ploidy
        self.W = 2 if kind == "w2" else 1
        self.calling = kind == "call"

    @property
    def id(self):
        return "%s-ploidy%d" % (self.kind, self.K)

    def hap(self, i):
        """Symbol i, distinct for distinct i >= 0.  w1: symbol 0 is the word 0, the others spread over all 64 bits (every other
        one above 2^63).  w2: five high words (0 and one above 2^63 among them) by i % 5 over low words by i // 5, so symbols share
        one word with many others.  call: allele i."""
        if self.kind == "call":
            return i
        if self.kind == "w1":
            return (i * 0x9E3779B97F4A7C15) & MASK64
        hi = (0, 1, 0x8000000000000001, 0x0123456789ABCDEF, MASK64)[i % 5]
        lo = ((i // 5) * 0xD1B54A32D192ED03) & MASK64
        return (hi << 64) | lo

    def junk(self, j):
        """States for the burnt part, of symbols no case uses."""
        return self.state([100000 + j])

    def state(self, syms, v=0):
        """The genotype over the distinct symbols `syms`, every one present, the copies beyond one each by composition v of the
        ploidy (see compositions)."""
        return self.state_of([self.hap(i) for i in syms], v)

    def state_of(self, haps, v=0):
        m = len(haps)
        assert 1 <= m <= self.K and len(set(haps)) == m
        comps = compositions(self.K, m)
        c = comps[v % len(comps)]
        out = []
        for h, n in zip(haps, c):
            out += [h] * n
        return tuple(sorted(out))

    def dosages(self, m):
        """How many different genotypes one support of m haplotypes has at this ploidy."""
        return len(compositions(self.K, m))


def compositions(K, m):
    """The ways to give m haplotypes K copies, each at least one, in lexicographic order (at most the first 16)."""
    out = []
    for cuts in combinations(range(1, K), m - 1):
        edges = (0,) + cuts + (K,)
        out.append(tuple(edges[i + 1] - edges[i] for i in range(m)))
        if len(out) == 16:
            break
    return out


FORMS = [Form("w1", 2), Form("w1", 4), Form("w1", 8), Form("w2", 3), Form("w2", 10), Form("w2", 15),
         Form("call", 2), Form("call", 4), Form("call", 8)]


class Launch(object):
    """One batch call and one listed call over the same units.  units: [(ploidy, [chains][steps] states)], the burnt part
    included; max_states: rows of the batch call's per-state outputs; cap / unit_list: the listed call's table and list (None: a
    table of min(N, what the LDS holds) states, every unit in descending order); codes: {unit: the MCI code the unit is built for}."""

    def __init__(self, name, form, units, steps, chains, burn, threshold=0.6, ploidy_max=None, max_states=16, cap=None, unit_list=None,
                 codes=None):
        self.name, self.form, self.units = name, form, units
        self.steps, self.chains, self.burn, self.threshold = steps, chains, burn, threshold
        self.ploidy_max = form.K if ploidy_max is None else ploidy_max
        self.max_states, self.cap = max_states, cap
        self.unit_list = list(range(len(units) - 1, -1, -1)) if unit_list is None else unit_list
        self.codes = codes or {}
        for K, chs in units:
            assert len(chs) == chains and all(len(c) == steps for c in chs), name
            assert all(len(s) == K for c in chs for s in c), name
        assert 2 <= len(units) <= 5 and 0 <= burn < steps

    @property
    def n_obs(self):
        return self.chains * (self.steps - self.burn)

    def burnt(self, u):
        return [c[self.burn:] for c in self.units[u][1]]


def _launch(name, form, bodies, burn=2, ploidies=None, **kw):
    """bodies: per unit [chains] lists of states after burn-in; every chain gets `burn` junk states in front."""
    units = []
    j = 0
    for u, chs in enumerate(bodies):
        f = form if ploidies is None else Form(form.kind, ploidies[u])
        full = []
        for c in chs:
            full.append([f.junk(j + i) for i in range(burn)] + list(c))
            j += burn
        units.append((f.K, full))
    steps = len(units[0][1][0])
    return Launch(name, form, units, steps, len(bodies[0]), burn, **kw)


def _spread(seq, counts):
    """A chain in which seq[i] occurs counts[i] times, first appearances in the order of seq, the copies interleaved."""
    left = list(counts)
    out = []
    while any(left):
        for i, s in enumerate(seq):
            if left[i]:
                out.append(s)
                left[i] -= 1
    return out


# ---- the cases ----
def one_state(f):
    a, b, c = f.state([0]), f.state([1, 2] if f.K >= 2 else [1]), f.state([3])
    return [_launch("one-state/N=1", f, [[[a]], [[b]], [[c]]], burn=0),
            _launch("one-state/N=14", f, [[[a] * 7, [a] * 7], [[b] * 7, [b] * 7]], burn=3)]


def tail(f):
    out = []
    for n in (1, 63, 64, 65, 130):
        chains = 2 if n == 130 else 1
        per = n // chains
        bodies = []
        for u in range(3):
            pool = [f.state([u, 10 + i]) for i in range(4)]
            flat = [pool[(i * (u + 2)) % 4 if i % 7 else 0] for i in range(n)]
            flat[-1] = f.state([20 + u])  # the last state of the merged order occurs nowhere else
            bodies.append([flat[c * per:(c + 1) * per] for c in range(chains)])
        out.append(_launch("tail/N=%d" % n, f, bodies, burn=1))
    return out


def twins_in_a_batch(f):
    A, B, C_, D, E = (f.state([i]) for i in range(5))
    # unit 0: B is new at lanes 3 and 40 of the first batch; C at lanes 3 and 40 of the second; D then E new in the third.  The new
    # states' counts tie, so the ranks show the order of first appearance
    u0 = [A] * 192
    u0[3] = u0[40] = B
    u0[64 + 3] = u0[64 + 40] = C_
    u0[128 + 10], u0[128 + 20] = D, E
    u0[128 + 30], u0[128 + 31] = E, D
    # unit 1: the same with E before D, and B / C at lanes 0 and 63
    u1 = [A] * 192
    u1[0] = u1[63] = B
    u1[64] = u1[127] = C_
    u1[128 + 10], u1[128 + 20] = E, D
    u1[128 + 30], u1[128 + 31] = E, D
    # unit 2: every lane of the first batch a new state, each twice (lanes i and 32 + i)
    pool = [f.state([i, 50] if f.K >= 2 else [i]) for i in range(32)]
    u2 = pool + pool + [A] * 128
    return [_launch("twins-in-a-batch", f, [[u0], [u1], [u2]], burn=0, max_states=40)]


def tied_counts(f):
    s = [f.state([i, 7] if f.K >= 2 else [i]) for i in range(5)]
    bodies = [[_spread(s, [3] * 5), _spread(s[::-1], [3] * 5)],                 # merged first appearance: 0 1 2 3 4
              [_spread([s[2], s[0], s[4]], [4, 4, 4]) + [s[1]] * 3, [s[3]] * 7 + [s[1]] * 4 + [s[0]] * 4],   # 8, 7, 7, 4, 4
              [[s[4]] * 15, _spread([s[3], s[1], s[0], s[2]], [5, 5, 3, 2])]]
    return [_launch("tied-counts", f, bodies)]


def tied_supports(f):
    # unit 0: one-genotype supports with equal counts: the first rank wins
    x, y, z = f.state([0, 1]), f.state([2, 3]), f.state([4])
    bodies = [[_spread([x, y, z], [6, 6, 4]), _spread([z, y, x], [6, 5, 5])]]   # x 11, y 11, z 10 of 32
    w = [f.state([5]), f.state([6]), f.state([8])]
    if f.dosages(2) >= 2:
        # units 1, 2: supports {0, 1} and {2, 3} with the count sequences (5, 3) and (5, 3): bit-equal sums, above everything else
        x1, x2, y1, y2 = f.state([0, 1], 0), f.state([0, 1], 1), f.state([2, 3], 0), f.state([2, 3], 1)
        rest = _spread([z] + w, [4, 4, 4, 4])
        bodies.append([_spread([x1, y1, x2, y2], [5, 5, 3, 3]), rest])
        bodies.append([_spread([y2, x2, y1, x1], [3, 3, 5, 5]), rest])
        # unit 3: support {0, 1} (4 + 4 of 32) beats the most frequent genotype z (6): the mode genotype is not rank 0
        bodies.append([_spread([z, x1, x2, y1], [6, 4, 4, 2]), _spread(w, [5, 5, 4]) + [y2, y2]])
    else:
        bodies.append([_spread([z, y, x], [4, 6, 6]), _spread([x, z, y], [5, 6, 5])])   # the same with z first
    return [_launch("tied-supports", f, bodies)]


def dosage_only(f):
    """{a,a,b,b}, {a,b,b,b} and {a,a,a,b} are one support; {a,a,a,a} is another (and the single most frequent genotype)."""
    if f.dosages(2) < 2:
        return []
    n = min(3, f.dosages(2))
    ab = [f.state([0, 1], v) for v in range(n)]
    aa, ac = f.state([0]), f.state([0, 2])
    cnt = [5, 4, 3][:n]
    T = sum(cnt)   # every chain has T + 9 states
    bodies = [[_spread([aa] + ab + [ac], [7] + cnt + [2]), _spread(ab[::-1] + [aa, ac], cnt[::-1] + [6, 3])],   # aa 13 < the support's 2 T
              [_spread(ab + [ac, aa], cnt + [6, 3]), _spread([ac] + ab + [aa], [1] + cnt + [8])],
              [_spread([aa, ac] + ab, [T + 8 - 2 * n, 1] + [2] * n), [aa] * (T + 9 - 3 * n) + _spread(ab, [3] * n)]]   # here {a} wins
    return [_launch("dosage-only", f, bodies)]


def _word_only(f, name, x, y, y2, z):
    assert f.kind == "w2"
    S = f.state_of
    # posterior: the supports {x, y} and {x, y'} are different; merged they would outweigh {z}
    post = [[_spread([S([z]), S([x, y]), S([x, y2], 0), S([x, y2], 1)], [5, 4, 3, 3]), _spread([S([x, y]), S([y, y2]), S([y]), S([y2])], [6, 4, 3, 2])],
            [_spread([S([x, y2]), S([x, y], 1), S([x, y], 0), S([z, y])], [5, 4, 4, 2]), _spread([S([y2]), S([y]), S([y, y2])], [7, 7, 1])]]
    out = [_launch(name + "/supports", f, post)]
    # incongruence: codes 0, 1 and 2 among haplotypes that differ in that one word
    mci = [[[S([x, y], 0)] * 6, [S([x, y], 1)] * 6],
           [[S([x, y, y2])] * 6, [S([x, y])] * 6],
           [[S([x, y])] * 6, [S([x, y2])] * 6],
           [[S([y])] * 6, [S([y2])] * 6]]
    out.append(_launch(name + "/mci", f, mci, codes={0: 0, 1: 1, 2: 2, 3: 2}))
    return out


def high_word_only(f):
    if f.kind != "w2":
        return []
    lo = 0x00FF00FF00FF00FF
    return _word_only(f, "high-word-only", (5 << 64) | lo, (6 << 64) | lo, (0x8000000000000006 << 64) | lo, (9 << 64) | 77)


def low_word_only(f):
    if f.kind != "w2":
        return []
    hi = 0x0F0F0F0F0F0F0F0F << 64
    return _word_only(f, "low-word-only", hi | 5, hi | 6, hi | 0x8000000000000006, (9 << 64) | 77)


def _many(f, n, first=0):
    """n distinct states."""
    if f.K >= 2:
        return [f.state([0, first + 1 + i]) for i in range(n)]
    return [f.state([first + 1 + i]) for i in range(n)]


def _full_table(f, table, per_chain, name, **kw):
    cap = table
    assert per_chain >= cap + 8
    s = _many(f, cap + 1)
    half = cap // 2

    def chain(states):
        return (states + [states[0]] * per_chain)[:per_chain]

    bodies = [[chain(s[:half]), chain(s[half:cap])],              # cap states in all: the table is full, nothing is lost
              [chain(s[:half]), chain(s[half:cap + 1])],          # one more
              [chain(s[:3]), chain(s[:cap + 1][::-1])],           # the second chain alone visits cap + 1
              [chain(s[:cap]), chain(s[:cap][::-1])]]             # each chain fills the table by itself
    return _launch(name, f, bodies, burn=4, max_states=8, **kw)


def full_table(f):
    return [_full_table(f, BATCH_CAP, 560, "full-table/batch"), _full_table(f, LISTED_CAP, 90, "full-table/listed", cap=LISTED_CAP)]


def truncated(f):
    """max_states = 4 over 9 distinct states; the mode support is two dosages (6 + 5 of 70) ranked 5 and 6 behind five genotypes of 10."""
    if f.dosages(2) < 2:
        return []
    singles = [f.state([10 + i]) for i in range(5)]
    d0, d1 = f.state([0, 1], 0), f.state([0, 1], 1)
    e0, e1 = f.state([2]), f.state([3])
    seq = singles + [d0, d1, e0, e1]
    cnt = [10] * 5 + [6, 5, 3, 6]
    flat = _spread(seq, cnt)
    flat2 = _spread(seq[::-1], cnt[::-1])
    assert len(flat) == 70
    return [_launch("truncated", f, [[flat[:35], flat[35:]], [flat2[:35], flat2[35:]]], max_states=4, cap=8, codes={})]


def ragged_ploidy(f):
    """Units of ploidy 2, 4, 3 under ploidy_max 4 (3, 11, 15 under 15 at two words); then under a ploidy_max that refuses one."""
    if f.K not in (4, 15):
        return []
    ploidies, low = ((2, 4, 3), 3) if f.K == 4 else ((3, 11, 15), 11)
    bodies = []
    for u, K in enumerate(ploidies):
        g = Form(f.kind, K)
        a, b, c = g.state([u, 1 + u]), g.state([u, 1 + u], 1), g.state([7])
        bodies.append([_spread([a, b, c], [4, 3, 2]), _spread([c, a], [5, 4])])
    return [_launch("ragged-ploidy/all-fit", f, bodies, ploidies=ploidies),
            _launch("ragged-ploidy/one-above", f, bodies, ploidies=ploidies, ploidy_max=low)]


def listed_subset(f):
    bodies = []
    for u in range(5):
        s = _many(f, u + 2, first=10 * u)
        bodies.append([_spread(s, list(range(u + 2, 0, -1))) + [s[0]] * (15 - (u + 2) * (u + 3) // 2 + 6), [s[-1]] * 10 + [s[0]] * 11])
    return [_launch("listed-subset", f, bodies, unit_list=[3, 1])]


def burn_edges(f):
    a, b = f.state([0]), f.state([1])
    bodies0 = [[[a] * 8 + [b] * 4, [b] * 12], [[b] * 12, [a] * 5 + [b] * 7]]
    last = [[[a], [b]], [[b], [b]], [[a], [a]]]
    return [_launch("burn/none", f, bodies0, burn=0), _launch("burn/all-but-one", f, last, burn=11)]


def mci_codes(f):
    """The codes of both rules, three chains, threshold 0.6.  A chain `below` spreads over four supports of 25 % each."""
    K = f.K
    S = f.state
    below = _spread([S([20]), S([21]), S([22]), S([23])], [2, 2, 2, 2])
    full = lambda s: [s] * 8  # noqa: E731
    wide = list(range(K))                   # K distinct haplotypes: the whole ploidy named
    sub = wide[:-1] if K > 1 else wide      # a strict subset of them
    bodies, codes = [], {}

    def add(chs, code):
        codes[len(bodies)] = code
        bodies.append(chs)

    add([full(S(wide)), full(S(wide)), full(S(wide))], 0)                              # the chains agree
    add([full(S(wide)), full(S(sub)), full(S(wide))], 1)                               # disagree, the union equals the first
    add([full(S(sub)), full(S(wide)), full(S(sub))], 1 if f.calling else 2)            # ... the first is the smaller one
    add([full(S(wide)), full(S(wide[:-1] + [K])), below], 2)                           # together K + 1 are named
    add([below, full(S(wide)), full(S(sub))], 1)                                       # the first kept chain is not chain 0
    l1 = [_launch("mci-codes/a", f, bodies, codes=codes)]
    bodies, codes = [], {}
    add([below, below, below], 0)                                                      # no chain is kept
    add([below, full(S(wide)), below], 0)                                              # one is
    add([below, full(S([0])), full(S([1]))], 1 if (f.calling and K > 1) else 2)        # {a} vs {b}: union 2 > 1; two alleles named
    if f.dosages(2) >= 2:
        add([full(S([0, 1], 0)), full(S([0, 1], 1)), below], 1 if f.calling else 0)    # {a,a,b,b} vs {a,b,b,b}: what `calling` decides
    if K >= 3:
        add([below, full(S([0, 1])), full(S([0, 2]))], 1 if f.calling else 2)          # union 3 > 2, but not above the ploidy
    return l1 + [_launch("mci-codes/b", f, bodies, codes=codes)]


def threshold_edge(f):
    """One-genotype supports whose count / N is the threshold itself (3 of 5 at 0.6, 3 of 4 at 0.75) or one count below it."""
    a, b, o = f.state([0]), f.state([1]), [f.state([10 + i]) for i in range(4)]
    out = []
    for n, thr in ((5, 0.6), (4, 0.75)):
        at = lambda s, i: _spread([s, o[i], o[i + 1]], [3, 1, n - 4]) if n == 5 else _spread([s, o[i]], [3, 1])  # noqa: E731
        under = lambda s, i: _spread([s, o[i], o[i + 1]], [2, 2, n - 4]) if n == 5 else _spread([s, o[i]], [2, 2])  # noqa: E731
        bodies = [[at(a, 0), at(b, 2)],          # both kept: they disagree
                  [at(a, 0), under(b, 2)],       # the second is not kept: nothing to disagree with
                  [under(a, 0), at(b, 2)]]
        code = 1 if (f.calling and f.K > 1) else 2
        out.append(_launch("threshold-edge/%d-of-%d" % (3, n), f, bodies, burn=1, threshold=thr, codes={0: code, 1: 0, 2: 0}))
    return out


def chains_32(f):
    """POST_MAX_CHAINS chains of 20 steps: every chain its own support of `ploidy` haplotypes (the far end of sets / nset)."""
    if f.K not in (8, 15):
        return []
    K = f.K
    own = [[f.state(list(range(c, c + K)))] * 14 + [f.state([c])] * 6 for c in range(POST_MAX_CHAINS)]
    same = [[f.state(list(range(K)))] * 20 for _ in range(POST_MAX_CHAINS)]
    last = [_spread([f.state([30 + 4 * c + i]) for i in range(4)], [5] * 4) for c in range(POST_MAX_CHAINS - 2)]
    last += [[f.state(list(range(K)))] * 20, [f.state(list(range(1, K + 1)))] * 20]
    return [_launch("32-chains", f, [own, same, last], burn=0, max_states=64, codes={0: 2, 1: 0, 2: 2})]


CASES = {
    "one-state": one_state,
    "tail": tail,
    "twins-in-a-batch": twins_in_a_batch,
    "tied-counts": tied_counts,
    "tied-supports": tied_supports,
    "dosage-only": dosage_only,
    "high-word-only": high_word_only,
    "low-word-only": low_word_only,
    "full-table": full_table,
    "truncated": truncated,
    "ragged-ploidy": ragged_ploidy,
    "listed-subset": listed_subset,
    "burn": burn_edges,
    "mci-codes": mci_codes,
    "threshold-edge": threshold_edge,
    "32-chains": chains_32,
}


def launches(name):
    """Every launch of a case, over the forms it applies to."""
    out = []
    for f in FORMS:
        out += CASES[name](f)
    return out


def all_launches():
    return [l for name in CASES for l in launches(name)]
