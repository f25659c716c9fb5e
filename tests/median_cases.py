"""The edges of the exact median of positives (qingdai_amd/csrc/qd_reduce.hip), one case per edge, and the form report
(Device.median_state) each call of a case must give.  Shared by tests/test_gpu_median_forms.py (device against numpy, report against
prediction) and tests/test_median_cases_cpu.py (every case sits on the edge it is named for; every form is reached).  Test
infrastructure only.  Every field is a function of the case's shape and a seed; nothing is stored.

The forms (FORMS below):
  1    first call of a site (k_sel_pass x2, k_sel_collect, k_sel_final, k_med_seed); every call with QD_MEDIAN_PREDICT=0 or site -1
  2a   windowed (k_med_hist, k_med_scan_bracket, k_med_final), the list of <= 4096 candidates in LDS
  2b   windowed, > 4096 candidates: the list in global memory, fixed digits
  2c   windowed, the finisher's ranks are not in the list: it selects from the field itself
  3    the pair chain (k_med_hist2, k_med_scan_bracket2, k_med_final2); each job is 2a, 2b or 2c as well
  4a   bands, windowed: gathered segments compacted into LDS (<= 4096 candidates in all)
  4b   bands, windowed: gathered segments read as world x cap slots (> 4096 candidates)
  4c   bands, windowed: miss flag (a band over its 4092 candidates, or ranks outside the list): six all-reduced passes, re-seed
  4-first  bands, first call of a site, QD_MEDIAN_PREDICT=0, site -1: six all-reduced passes
  5    transform 1, max(0, -(x - tparam)), on top of any of the above

The window arithmetic restated (qd_med_window_base, qd_med_scan, qd_med_final_body):
  base = bits(centre) - (4 << 52), clamped at 0 (centre = 1.0 while the site has no valid centre); 2048 bins of 2^44 patterns;
  top = base + 2^55.  Ranks k1 = (m - 1) // 2, k2 = m // 2 of the m positives.  Both ranks inside the window: the bracket is the
  bins of the two ranks.  k2 below the window: [1, base - 1]; k1 above: [top, DBL_MAX]; anything else: [1, DBL_MAX].  The
  finisher hits when the list holds both ranks: c_lo <= k1 and k2 < c_lo + M (c_lo = positives below the bracket).  +inf is never
  listed (the bracket ends at DBL_MAX), so a rank that is +inf is the one way into 2c on a whole-globe handle.

Shapes the issue named that the library cannot take as named:
  511 ... 600 candidates in the rows of ONE workgroup: QD_MED_BLOCKS below 16 is ignored, so at (17, 256) a workgroup has at most
  two rows (512 cells).  Those cases run at (17, 640): 17 workgroups of one 640-cell row each.
  One band at 4092 / 4093 candidates on three bands: a band of (40, 256) has 14 x 256 = 3584 cells.  World 3 runs them at (40, 320).
  Bands of (40, 256) with the default halo of 12 rows are refused on two bands (20 + 24 rows > 40): the groups take halo = 6.
"""
import numpy as np

BINS, WSHIFT, LDS_LIST, WG_STAGE, BAND_CAP, SITES = 2048, 44, 4096, 512, 4092, 4
FOUR = 4 << 52
MAXB = 0x7FEFFFFFFFFFFFFF                     # DBL_MAX
INFB = 0x7FF0000000000000
TINY = 5e-324
DBL_MAX = float(np.finfo(np.float64).max)
BAND_HALO = 6

FORMS = ("1", "2a", "2b", "2c", "3", "4a", "4b", "4c", "4-first", "5")


def bits(v):
    return int(np.float64(v).view(np.uint64))


def from_bits(b):
    return float(np.uint64(b).view(np.float64))


def med_value_kernel(x, transform, tparam):
    """qd_med_value: transform 1 is qd_max(0.0, -(x - tparam)), qd_max = np.maximum"""
    x = np.asarray(x, dtype=np.float64)
    if transform != 1:
        return x
    with np.errstate(all="ignore"):
        d = x - np.float64(tparam)
        return np.maximum(0.0, -d)


def med_value_physics(div, D_crit):
    """physics.py:296, as it stands there"""
    with np.errstate(all="ignore"):
        pos = np.maximum(0.0, -(div - float(D_crit)))
    return pos


def expected(x, dflt, transform=0, tparam=0.0):
    """np.median(t(x)[t(x) > 0]) in float64, or dflt"""
    with np.errstate(all="ignore"):
        v = med_value_kernel(x, transform, tparam)
        pos = v[v > 0]
        return float(np.median(pos)) if pos.size else float(dflt)


def same(a, b):
    """bit equality of two medians (inf == inf; a median of positives is never NaN or -0.0)"""
    return (np.isinf(a) and np.isinf(b) and a > 0 and b > 0) or a == b


def band_ranges(n_lat, world):
    base, rem = divmod(int(n_lat), int(world))
    out, r = [], 0
    for k in range(world):
        n = base + (1 if k < rem else 0)
        out.append((r, n))
        r += n
    return out


# ------------------------------------------------------------------------------------------------------------------ the model
class Site:
    def __init__(self):
        self.centre, self.valid, self.seen = 0.0, False, False
        self.hits = self.misses = self.list_len = self.count = self.lo_bits = self.hi_bits = self.calls = 0

    def report(self):
        return dict(centre=self.centre, valid=self.valid, hits=self.hits, misses=self.misses, list_len=self.list_len, count=self.count,
                    lo_bits=self.lo_bits, hi_bits=self.hi_bits, calls=self.calls)


class Model:
    """The host logic of qd_median_positive_dev / qd_median_pair_dev and the decisions of its kernels, on one handle (world = 0)
    or one group of band handles (every band keeps the same site state)."""

    def __init__(self, shape, predict=True, world=0, med_blocks=256):
        self.shape, self.predict, self.world = tuple(shape), predict, world
        self.sites = [Site() for _ in range(SITES)]
        self.nby = min(shape[0], med_blocks if med_blocks >= 16 else 256)       # workgroups of a whole-globe pass, one per row stride
        self.ranges = band_ranges(shape[0], world) if world else None

    @staticmethod
    def _exact(v):
        with np.errstate(all="ignore"):
            pos = np.sort(v[v > 0])
            m = pos.size
            if m == 0:
                return None, 0
            v1, v2 = pos[(m - 1) // 2], pos[m // 2]
            return float(v1 if m & 1 else (v1 + v2) / np.float64(2.0)), m

    def _window(self, v, S):
        """k_med_hist + qd_med_scan + the collecting pass: bracket, list, counts"""
        with np.errstate(all="ignore"):
            posmask = v > 0
        pos = np.ascontiguousarray(v[posmask])
        b = pos.view(np.uint64)
        m = int(pos.size)
        cb = bits(S.centre if S.valid else 1.0)
        base = cb - FOUR if cb > FOUR else 0
        top = base + (BINS << WSHIFT)
        W = dict(m=m, base=base, top=top, scan_ok=False, lo_bits=1, hi_bits=MAXB, M=0, c_lo=0, k1_bin=None, k2_bin=None,
                 wg=[], band_M=[])
        if m == 0:
            return W
        below = int((b < np.uint64(base)).sum())
        total = int(((b >= np.uint64(base)) & (b < np.uint64(top))).sum())
        k1, k2 = (m - 1) // 2, m // 2
        sb = np.sort(b)
        W["k1_bin"], W["k2_bin"] = (int(sb[k1]) - base) >> WSHIFT, (int(sb[k2]) - base) >> WSHIFT      # floor: -1 = just below
        lo_b, hi_b = 1, MAXB
        if S.valid and k1 >= below and k2 < below + total:
            W["scan_ok"] = True
            lo_b = base + (W["k1_bin"] << WSHIFT)
            hi_b = base + ((W["k2_bin"] + 1) << WSHIFT) - 1
        elif S.valid:
            if k2 < below:
                hi_b = (base - 1) & (2 ** 64 - 1)                 # unsigned, as in the kernel (then clipped)
            elif k1 >= below + total:
                lo_b = top
        lo_b, hi_b = max(lo_b, 1), min(hi_b, MAXB)
        lo, hi = from_bits(lo_b), from_bits(hi_b)
        with np.errstate(all="ignore"):
            cand = posmask & (v >= lo) & (v <= hi)
            W["c_lo"] = int((posmask & (v < lo)).sum())
        per_row = cand.sum(axis=1)
        W.update(lo_bits=lo_b, hi_bits=hi_b, M=int(cand.sum()), k1=k1, k2=k2)
        W["wg"] = sorted((int(per_row[w::self.nby].sum()) for w in range(self.nby)), reverse=True)
        if self.world:
            W["band_M"] = [int(per_row[r0:r0 + n].sum()) for r0, n in self.ranges]
        return W

    def _one(self, x, dflt, transform, tparam, site, chain):
        v = np.ascontiguousarray(med_value_kernel(x, transform, tparam)).reshape(self.shape)
        value, m = self._exact(v)
        value = float(dflt) if value is None else value
        P = dict(value=value, m=m, form=None, hit=None, miss=False, allreduces=0, M=None, transform=transform)
        windowed = self.predict and 0 <= site < SITES
        S = self.sites[site] if windowed else None
        if not windowed or not S.seen:
            P["form"] = "4-first" if self.world else "1"
            P["allreduces"] = 6 if self.world else 0
            if windowed:
                S.seen, S.centre, S.valid = True, value, m > 0
        else:
            W = self._window(v, S)
            P.update(W)
            S.lo_bits, S.hi_bits = W["lo_bits"], W["hi_bits"]
            if self.world:
                P["allreduces"] = 2
                over = any(c > BAND_CAP for c in W["band_M"])
                M = sum(min(c, BAND_CAP) for c in W["band_M"])
                P["M"] = M
            else:
                over, M = False, W["M"]
            if m == 0:
                P["form"], P["hit"] = "none", None
                S.valid = False
            else:
                hit = (not over) and W["c_lo"] <= W["k1"] and W["k2"] < W["c_lo"] + M
                P["hit"] = hit
                if self.world and not hit:
                    P["form"], P["miss"], P["allreduces"] = "4c", True, 8
                    S.centre, S.valid = value, True
                else:
                    big = M > LDS_LIST
                    P["form"] = ("4b" if big else "4a") if self.world else ("2c" if not hit else ("2b" if big else "2a"))
                    S.calls += 1
                    S.centre, S.valid, S.list_len, S.count = value, True, M, m
                    if hit:
                        S.hits += 1
                    else:
                        S.misses += 1
        P["chain"] = chain
        P["report"] = S.report() if S is not None else None
        return P

    def single(self, x, dflt, transform=0, tparam=0.0, site=0):
        return self._one(x, dflt, transform, tparam, site, "single")

    def pair(self, job0, job1):
        assert not self.world and self.predict and job0["site"] != job1["site"]
        assert self.sites[job0["site"]].seen and self.sites[job1["site"]].seen, "the seam refuses a pair before both sites have a window"
        return [self._one(j["x"], j["dflt"], j.get("transform", 0), j.get("tparam", 0.0), j["site"], "pair") for j in (job0, job1)]


def forms_of(P):
    """the rows of the table of forms a predicted call reaches"""
    out = set()
    if P["form"] in FORMS:
        out.add(P["form"])
    if P["chain"] == "pair":
        out.add("3")
    if P["transform"] == 1:
        out.add("5")
    return out


# ------------------------------------------------------------------------------------------------------------------ fields
def junk(n):
    """non-positive filler: +0, -0, a negative, NaN, -inf in turn"""
    return np.resize(np.array([0.0, -0.0, -2.5, np.nan, -np.inf]), n)


def field(shape, seed, values, rows=None, fill=None):
    """`values` on cells drawn by `seed` (inside `rows` when given), the filler everywhere else"""
    n_lat, n_lon = shape
    x = junk(n_lat * n_lon) if fill is None else np.full(n_lat * n_lon, fill, dtype=np.float64)
    values = np.asarray(values, dtype=np.float64).ravel()
    cells = np.arange(n_lat * n_lon) if rows is None else np.concatenate([np.arange(r * n_lon, (r + 1) * n_lon) for r in rows])
    assert values.size <= cells.size, (values.size, cells.size)
    r = np.random.default_rng(seed)
    x[r.permutation(cells)[:values.size]] = values
    return x.reshape(shape)


def spread(seed, n, centre, sigma=1.0):
    """n positive values, log-normal around `centre`"""
    with np.errstate(over="ignore"):                             # (around 1e308 a few of them are inf: meant)
        return centre * np.exp(np.random.default_rng(seed).normal(0.0, sigma, n))


def seed_field(shape, seed, c):
    """three positives with median exactly c: the seeding call of a site"""
    d = min(1 << 50, bits(c) // 2)                               # (a subnormal centre has few patterns below it)
    return field(shape, seed, [from_bits(bits(c) - d), c, from_bits(bits(c) + d)])


def single(x, dflt=1e-6, transform=0, tparam=0.0, site=0, **edge):
    return dict(op="single", x=x, dflt=dflt, transform=transform, tparam=tparam, site=site, edge=edge)


def pair(job0, job1, edge0=None, edge1=None):
    return dict(op="pair", jobs=(job0, job1), edges=(edge0 or {}, edge1 or {}))


def job(x, dflt=1e-6, transform=0, tparam=0.0, site=0):
    return dict(x=x, dflt=dflt, transform=transform, tparam=tparam, site=site)


CASES = {}


def case(cid, shape, env=None, world=0, transports=(None,), three_way=False, why=""):
    def reg(fn):
        CASES[cid] = dict(id=cid, shape=shape, env=dict(env or {}), world=world, transports=transports, three_way=three_way, why=why,
                          build=lambda: fn(shape))
        return fn
    return reg


def predict_case(C, calls=None, predict=True):
    """the model's predictions for every call of a case, in order (a pair gives two)"""
    calls = C["build"]() if calls is None else calls
    mb = int(C["env"].get("QD_MED_BLOCKS", 256))
    M = Model(C["shape"], predict=predict and C["env"].get("QD_MEDIAN_PREDICT") != "0", world=C["world"], med_blocks=mb)
    out = []
    for c in calls:
        if c["op"] == "single":
            out.append([M.single(c["x"], c["dflt"], c["transform"], c["tparam"], c["site"])])
        else:
            out.append(M.pair(*c["jobs"]))
    return calls, out


# ------------------------------------------------------------------------------------------------------------------ geometry
GEOMETRY = {(5, 4): "the smallest handle", (5, 63): "partial wave", (7, 65): "partial wave, one lane past",
            (6, 257): "one thread past a block",
            (5, 2051): "second column batch of k_sel_pass, k_sel_collect, k_med_hist, k_med_scan_bracket; batch-to-next-row hand-over",
            (37, 72): "QD_MED_BLOCKS=16: workgroups that walk three rows, the last row ragged",
            (17, 256): "the grid of the 4096 cases"}


def _geometry(shape):
    n = shape[0] * shape[1]
    npos = n - max(2, n // 10)                                   # a tenth of the cells non-positive
    npos -= npos & 1                                             # even: two middles
    a = spread(shape[1], npos, 3.0)
    calls = [single(field(shape, 1, a), form="1"),
             single(field(shape, 2, a * 1.01), form="2a", hit=True, scan_ok=True),
             single(field(shape, 3, np.concatenate([a[:npos // 2 - 1], np.full(npos // 2 + 1, np.inf)])), form="2c", hit=False, m=npos),
             # the centre is inf now: the ranks lie below the window, the lower side is every positive
             single(field(shape, 4, a * 0.99), form="2a" if npos <= LDS_LIST else "2b", hit=True, scan_ok=False, M=npos)]
    return calls


for _shape, _why in GEOMETRY.items():
    case(f"geometry/{_shape[0]}x{_shape[1]}", _shape, env={"QD_MED_BLOCKS": "16"} if _shape == (37, 72) else None, three_way=True,
         why=_why)(_geometry)


# ------------------------------------------------------------------------------------------------------------------ capacity
def _ties_in_bin(n):
    """n values of three distinct patterns inside the bin of 1.0"""
    return 1.0 + (np.arange(n) % 3) * 2.0 ** -30


def _capacity(M, extra_hi):
    def build(shape):
        vals = np.concatenate([_ties_in_bin(M), np.full(100, 0.25), np.full(extra_hi, 4.0)])
        return [single(seed_field(shape, 5, 1.0), form="1"),
                single(field(shape, 6, vals), form="2a" if M <= LDS_LIST else "2b", hit=True, M=M, m=M + 100 + extra_hi,
                       k1_bin=1024, k2_bin=1024),
                single(field(shape, 7, spread(7, 2000, 1.0)), form="2a", hit=True)]
    return build


for _M, _hi in ((4095, 100), (4095, 101), (4096, 100), (4096, 101), (4097, 100), (4097, 101)):
    case(f"capacity/list_{_M}_{'odd' if (_M + 100 + _hi) & 1 else 'even'}", (17, 256), three_way=True,
         why=f"{_M} tied candidates in the bracket: the LDS list against the global list")(_capacity(_M, _hi))


def _stage(counts):
    def build(shape):
        x = field(shape, 8, np.concatenate([np.full(50, 0.25), np.full(50, 4.0)]), rows=[0, 1, 2])
        for k, (row, n) in enumerate(counts):
            x[row] = field((1, shape[1]), 9 + k, 1.0 + np.arange(n) * 2.0 ** -40)[0]
        tot = sum(n for _, n in counts)
        return [single(seed_field(shape, 5, 1.0), form="1"),
                single(x, form="2a", hit=True, M=tot, wg_top=sorted((n for _, n in counts), reverse=True)),
                single(field(shape, 7, spread(7, 2000, 1.0)), form="2a", hit=True)]
    return build


for _n in (511, 512, 513, 600):
    case(f"capacity/stage_{_n}", (17, 640), three_way=True,
         why=f"{_n} candidates in one workgroup's row: the 512-entry LDS stage and the direct append")(_stage([(5, _n)]))
case("capacity/stage_600_600", (17, 640), three_way=True, why="two workgroups both over the stage")(_stage([(5, 600), (11, 600)]))


# ------------------------------------------------------------------------------------------------------------------ window
WSHAPE = (7, 65)
WCENTRE = 1.37


def _wbase(c):
    cb = bits(c)
    base = cb - FOUR if cb > FOUR else 0
    return base, base + (BINS << WSHIFT)


def _window_case(cid, centre, make, why, **edge):
    def build(shape):
        base, top = _wbase(centre)
        return [single(seed_field(shape, 11, centre), form="1"),
                single(field(shape, 12, make(base, top)), **edge),
                single(field(shape, 13, spread(13, 200, centre, 0.3)), hit=True)]
    case(f"window/{cid}", WSHAPE, three_way=True, why=why)(build)


def _inwin(n, k=14):
    return spread(k, n, WCENTRE, 0.2)


_window_case("bin0", WCENTRE, lambda b, t: np.concatenate([np.full(61, from_bits(b + 5)), _inwin(40)]),
             "the median in bin 0", form="2a", hit=True, scan_ok=True, k1_bin=0, k2_bin=0, M=61)
_window_case("div16", WCENTRE, lambda b, t: np.concatenate([np.full(61, WCENTRE / 16.0), _inwin(40)]),
             "the median exactly centre / 16: the first pattern of bin 0", form="2a", hit=True, scan_ok=True, k1_bin=0, k2_bin=0, M=61)
_window_case("below1", WCENTRE, lambda b, t: np.concatenate([np.full(61, from_bits(b - 1)), _inwin(40)]),
             "one pattern below bin 0: both ranks out on the lower side, hi_b = base - 1", form="2a", hit=True, scan_ok=False,
             k1_bin=-1, k2_bin=-1, M=61, lo_bits=1)
_window_case("bin2047", WCENTRE, lambda b, t: np.concatenate([np.full(61, from_bits(t - 1)), _inwin(40)]),
             "the median in bin 2047", form="2a", hit=True, scan_ok=True, k1_bin=2047, k2_bin=2047, M=61)
_window_case("times16", WCENTRE, lambda b, t: np.concatenate([np.full(61, WCENTRE * 16.0), _inwin(40)]),
             "the median exactly centre x 16: the first pattern above the window, lo_b = top", form="2a", hit=True, scan_ok=False,
             k1_bin=2048, k2_bin=2048, M=61, hi_bits=MAXB)
_window_case("straddle_up", WCENTRE, lambda b, t: np.concatenate([_inwin(50), np.full(50, from_bits(t + 7))]),
             "k1 in the window, k2 above it: every positive is a candidate", form="2a", hit=True, scan_ok=False, k1_bin=lambda k: 0 <= k < 2048,
             k2_bin=2048, M=100, lo_bits=1, hi_bits=MAXB)
_window_case("straddle_low", WCENTRE, lambda b, t: np.concatenate([np.full(50, from_bits(b - 9)), _inwin(50)]),
             "k1 below the window, k2 in it: every positive is a candidate", form="2a", hit=True, scan_ok=False, k1_bin=-1,
             k2_bin=lambda k: 0 <= k < 2048, M=100, lo_bits=1, hi_bits=MAXB)
_window_case("subnormal_centre", 7 * TINY, lambda b, t: TINY * np.arange(1, 42),
             "a subnormal centre: the base clamps to 0 and lo_b to 1", form="2a", hit=True, scan_ok=True, k1_bin=0, base=0, lo_bits=1, M=41)
_window_case("huge_centre", 1e308, lambda b, t: np.concatenate([np.linspace(1.1e308, 1.7e308, 41), np.full(20, np.inf)]),
             "a centre above DBL_MAX / 16: the window reaches past the pattern of inf", form="2a", hit=True, scan_ok=True,
             top=lambda t: t > INFB)
_window_case("huge_centre_inf", 1e308, lambda b, t: np.concatenate([np.linspace(1.1e308, 1.7e308, 20), np.full(41, np.inf)]),
             "the same with the median at inf, whose pattern has a bin: the bracket clips at DBL_MAX, the list misses", form="2c",
             hit=False, scan_ok=True, hi_bits=MAXB)


# ------------------------------------------------------------------------------------------------------------------ ranks and ties
def _ranks_case(cid, vals, why, **edge):
    def build(shape):
        return [single(seed_field(shape, 21, 1.0), form="1"), single(field(shape, 22, vals), form="2a", hit=True, **edge)]
    case(f"ranks/{cid}", (5, 63), three_way=True, why=why)(build)


_A, _B = 1.0, 1.0 + 2.0 ** -20
_ranks_case("m1", [1.1], "one positive", m=1, M=1)
_ranks_case("m2", [0.9, 1.2], "two positives", m=2, M=2)
_ranks_case("m3", [0.9, 1.2, 1.3], "three positives", m=3)
_ranks_case("run_ends_at_k1", [_A] * 5 + [_B] * 5, "the run of v1 ends at rank k1: v2 is the next larger value", m=10, value=(_A + _B) / 2)
_ranks_case("run_ends_past_k1", [_A] * 6 + [_B] * 4, "the run of v1 ends one past k1: v2 = v1", m=10, value=_A)
_ranks_case("neighbour_bins", [from_bits(bits(1.0) + (1 << 44) - 1)] * 5 + [from_bits(bits(1.0) + (1 << 44))] * 5,
            "the two middles in neighbouring bins", m=10, k1_bin=1024, k2_bin=1025, M=10)
_ranks_case("seven_binades", [0.07] * 5 + [9.0] * 5,
            "the two middles 7 binades apart inside the window: a wide bracket", m=10, M=10, scan_ok=True,
            k1_bin=lambda k: k < 1024 - 3 * 256, k2_bin=lambda k: k >= 1024 + 3 * 256)


# ------------------------------------------------------------------------------------------------------------------ values
def _values_case(cid, centre, vals, why, **edge):
    def build(shape):
        x = field(shape, 32, vals)
        return [single(seed_field(shape, 31, centre), form="1"), single(x, site=0, **edge), single(x, site=1, form="1"),
                single(x, site=-1, form="1")]
    case(f"values/{cid}", (6, 257), three_way=True, why=why)(build)


_values_case("extremes_no_inf_middle", 1.0, np.concatenate([spread(33, 600, 1.0), [TINY, TINY, DBL_MAX, np.inf, np.inf]]),
             "-0.0, negatives, NaN in the filler; the smallest subnormal, DBL_MAX and +inf present, neither middle inf", form="2a", hit=True)
_values_case("inf_upper_middle", 1.0, np.concatenate([spread(34, 300, 1.0), np.full(300, np.inf)]),
             "+inf as the upper middle, the lower one finite: numpy gives inf", form="2c", hit=False, m=600, isinf=True)
_values_case("inf_both_middles", 1.0, np.concatenate([spread(35, 299, 1.0), np.full(301, np.inf)]),
             "+inf as both middles", form="2c", hit=False, m=600, isinf=True)
_values_case("sum_overflows", 1.5e308, [1.0e308] * 4 + [1.6e308, 1.7e308] + [DBL_MAX] * 4,
             "two finite middles whose sum overflows: numpy gives inf", form="2a", hit=True, m=10, isinf=True)
_values_case("subnormal_median", 1.0, [TINY] * 3 + [1.0] * 2, "the median is the smallest subnormal", form="2a", hit=True, value=TINY)
_values_case("dblmax_median", 1.0, [DBL_MAX] * 3 + [1.0] * 2, "the median is DBL_MAX: the last pattern a bracket can hold", form="2a",
             hit=True, value=DBL_MAX, hi_bits=MAXB)


# ------------------------------------------------------------------------------------------------------------------ transform 1
def transform_field(shape, seed, tparam):
    r = np.random.default_rng(seed)
    x = r.normal(0.0, 2e-5, shape)
    flat = x.ravel()
    flat[r.permutation(flat.size)[:30]] = tparam                 # transformed 0: must not count
    flat[r.permutation(flat.size)[:7]] = np.nan
    return x


def _transform_case(site, tparam):
    def build(shape):
        x = transform_field(shape, 40 + site, tparam)
        return [single(x, transform=1, tparam=tparam, site=site, dflt=1e-12, form="1"),
                single(x * 1.003, transform=1, tparam=tparam, site=site, dflt=1e-12, form="2a", hit=True, scan_ok=True),
                single(np.full(shape, tparam), transform=1, tparam=tparam, site=site, dflt=1e-12, form="none", m=0, value=1e-12)]
    return build


for _site, _tp in ((1, 1e-5), (2, 0.0), (3, -3e-6)):
    case(f"transform/site{_site}_{'pos' if _tp > 0 else 'zero' if _tp == 0 else 'neg'}", (7, 65), three_way=True,
         why=f"max(0, -(x - tparam)) with tparam = {_tp}; entries equal to tparam do not count")(_transform_case(_site, _tp))


# ------------------------------------------------------------------------------------------------------------------ the pair chain
PSHAPE = (17, 256)


def _pair_case(cid, j0, j1, why, e0, e1):
    """sites 2 and 3 seeded at 1.0 and 1e-3, the pair, then a single call on each site"""
    def build(shape):
        a, b = j0(shape), j1(shape)
        a.setdefault("site", 2); b.setdefault("site", 3)
        return [single(seed_field(shape, 51, 1.0), site=2, form="1"), single(seed_field(shape, 52, 1e-3), site=3, form="1"),
                pair(job(**a), job(**b), e0, e1),
                single(field(shape, 53, spread(53, 3000, 1.0)), site=2, hit=True, form="2a"),
                single(field(shape, 54, spread(54, 3000, 1e-3)), site=3, hit=True, form="2a")]
    case(f"pair/{cid}", PSHAPE, why=why)(build)


def _hit(c, seed):
    return lambda shape: dict(x=field(shape, seed, spread(seed, 3000, c)))


def _missf(c, seed):
    return lambda shape: dict(x=field(shape, seed, np.concatenate([spread(seed, 1000, c), np.full(1001, np.inf)])))


_pair_case("hit_hit", _hit(1.0, 55), _hit(1e-3, 56), "both jobs served from their LDS lists", dict(form="2a", hit=True), dict(form="2a", hit=True))
_pair_case("hit_miss", _hit(1.0, 55), _missf(1e-3, 56), "job 1 selects from its field", dict(form="2a", hit=True), dict(form="2c", hit=False))
_pair_case("miss_hit", _missf(1.0, 55), _hit(1e-3, 56), "job 0 selects from its field", dict(form="2c", hit=False), dict(form="2a", hit=True))
_pair_case("none_hit", lambda shape: dict(x=junk(shape[0] * shape[1]).reshape(shape), dflt=0.125), _hit(1e-3, 56),
           "job 0 has no positive entry: its default, its predictor dropped", dict(form="none", m=0, value=0.125), dict(form="2a", hit=True))
_pair_case("transforms", lambda shape: dict(x=1e-5 - field(shape, 57, spread(57, 3000, 1.0), fill=0.0), transform=1, tparam=1e-5),
           _hit(1e-3, 56), "transform 1 on job 0, transform 0 on job 1", dict(hit=True), dict(form="2a", hit=True))
_pair_case("global_and_lds", lambda shape: dict(x=field(shape, 58, np.concatenate([_ties_in_bin(4097), np.full(100, 0.25), np.full(100, 4.0)]))),
           _hit(1e-3, 56), "job 0 over 4096 candidates (global list), job 1 in LDS", dict(form="2b", hit=True, M=4097), dict(form="2a", hit=True))


# ------------------------------------------------------------------------------------------------------------------ bands
BSHAPE = (40, 256)
TRANSPORTS = ("host", "peer")


def _rows_of(shape, world, r):
    r0, n = band_ranges(shape[0], world)[r]
    return list(range(r0, r0 + n))


def _band_fill(shape, world, counts, seed, lo=100, hi=100):
    """counts[r] tied candidates (the bin of 1.0) in band r; `lo` values below and `hi` above the bracket in band 0's first rows"""
    x = junk(shape[0] * shape[1]).reshape(shape)
    for r, n in enumerate(counts):
        rows = _rows_of(shape, world, r)
        if r == 0:
            rows = rows[2:]
        blk = field((len(rows), shape[1]), seed + r, _ties_in_bin(n))
        x[rows] = blk
    x[0:2] = field((2, shape[1]), seed + 9, np.concatenate([np.full(lo, 0.25), np.full(hi, 4.0)]))
    return x


def _band_case(cid, world, make, why, shape=BSHAPE, env=None, transports=TRANSPORTS, wrap=True):
    """the seeding call of site 0 (centre 1.0), the case's calls, then an ordinary call that must be a hit again"""
    def build(shp):
        if not wrap:
            return make(shp)
        return [single(seed_field(shp, 61, 1.0), form="4-first", allreduces=6)] + make(shp) + \
               [single(field(shp, 62, spread(62, 3000, 1.0, 0.5)), form="4a", hit=True, allreduces=2, miss=False)]
    case(f"bands{world}/{cid}", shape, env=env, world=world, transports=transports, why=why)(build)


def _dense(shape, seed, centre, sigma=0.3):
    """positives on 97 % of the cells: more than 4092 in the tallest band of either band shape"""
    return field(shape, seed, spread(seed, int(0.97 * shape[0] * shape[1]), centre, sigma))


def _split(total, world):
    return [total // world + (1 if k < total % world else 0) for k in range(world)]


for _w in (2, 3):
    _cap_shape = BSHAPE if _w == 2 else (40, 320)
    _band_case("compact_hit", _w, lambda s: [single(field(s, 63, spread(63, 6000, 1.0)), form="4a", hit=True, allreduces=2, miss=False)],
               "a hit whose gathered segments are compacted into LDS")
    _band_case("total_4096", _w, lambda s, w=_w: [single(_band_fill(s, w, _split(4096, w), 64), form="4a", hit=True, M=4096, allreduces=2)],
               "4096 candidates in all: the last list that is compacted")
    _band_case("total_4097", _w, lambda s, w=_w: [single(_band_fill(s, w, _split(4097, w), 65), form="4b", hit=True, M=4097, allreduces=2)],
               "4097 candidates in all: the segments are read as world x cap slots")
    _band_case("band_4092", _w, lambda s, w=_w: [single(_band_fill(s, w, [10] * (w - 1) + [4092], 66), form="4b", hit=True, miss=False,
                                                         band_max=4092, allreduces=2)],
               "one band at exactly its 4092 candidates", shape=_cap_shape)
    _band_case("band_4093", _w, lambda s, w=_w: [single(_band_fill(s, w, [10] * (w - 1) + [4093], 67), form="4c", hit=False, miss=True,
                                                         band_max=4093, allreduces=8)],
               "one band one over its capacity: miss flag, six passes, re-seed", shape=_cap_shape)
    _band_case("all_in_first", _w, lambda s, w=_w: [single(_band_fill(s, w, [900] + [0] * (w - 1), 68), form="4a", hit=True, allreduces=2)],
               "every candidate in band 0")
    _band_case("none_in_first", _w, lambda s, w=_w: [single(_band_fill(s, w, [0] + [700] * (w - 1), 69), form="4a", hit=True, allreduces=2)],
               "no candidate in band 0")
    _band_case("side_low_fits", _w, lambda s: [single(field(s, 70, np.concatenate([np.full(61, 1e-3), spread(70, 40, 1.0, 0.2)])),
                                                      form="4a", hit=True, scan_ok=False, k2_bin=lambda k: k < 0, allreduces=2)],
               "the ranks left the window on the lower side; the side fits the segments")
    _band_case("side_high_fits", _w, lambda s: [single(field(s, 71, np.concatenate([np.full(61, 1e3), spread(71, 40, 1.0, 0.2)])),
                                                       form="4a", hit=True, scan_ok=False, k1_bin=lambda k: k >= 2048, allreduces=2)],
               "the ranks left the window on the upper side; the side fits the segments")
    _band_case("side_low_overflows", _w, lambda s: [single(_dense(s, 72, 1e-4), form="4c", miss=True, scan_ok=False, allreduces=8)],
               "a window miss on the lower side with a band over its capacity", shape=_cap_shape)
    _band_case("side_high_overflows", _w, lambda s: [single(_dense(s, 73, 1e4), form="4c", miss=True, scan_ok=False, allreduces=8)],
               "a window miss on the upper side with a band over its capacity", shape=_cap_shape)
    _band_case("inf_rank", _w, lambda s: [single(field(s, 74, np.concatenate([spread(74, 300, 1.0), np.full(300, np.inf)])), form="4c",
                                                 miss=True, hit=False, isinf=True, allreduces=8)],
               "+inf as the upper middle: the gathered list cannot hold the rank")
    _band_case("none_then_some", _w, lambda s: [single(junk(s[0] * s[1]).reshape(s), dflt=0.5, form="none", m=0, value=0.5, allreduces=2, miss=False),
                                                single(_dense(s, 75, 1.0, 1.0), form="4c", miss=True, allreduces=8, lo_bits=1, hi_bits=MAXB)],
               "no positive anywhere drops the predictor; the next field overflows the unbounded bracket and re-seeds the site",
               shape=_cap_shape)
    _band_case("predict_off", _w, lambda s: [single(field(s, 76 + k, spread(76, 6000, 1.0 + 0.01 * k)), form="4-first", allreduces=6)
                                             for k in range(3)],
               "QD_MEDIAN_PREDICT=0: six all-reduced passes every call", env={"QD_MEDIAN_PREDICT": "0"}, wrap=False)
    _band_case("transform_site1", _w, lambda s: [single(transform_field(s, 77, 1e-5) * f, transform=1, tparam=1e-5 * f, site=1, dflt=1e-12,
                                                        **e) for f, e in ((1.0, dict(form="4-first", allreduces=6)),
                                                                          (1.003, dict(form="4a", hit=True, scan_ok=True, allreduces=2)))],
               "transform 1 at site 1 on the band forms", wrap=False)


def _drift(shape):
    base = field(shape, 80, spread(80, 7000, 2.0))
    r = np.random.default_rng(81)
    out = [single(base, form="4-first", allreduces=6)]
    for k in range(1, 20):
        out.append(single(base * (1.0 + 0.004 * k) * (1.0 + 1e-4 * r.normal(0, 1, shape)), form="4a", hit=True, allreduces=2))
    return out


case("bands3/drift20", BSHAPE, world=3, transports=("peer", "peer_nohooks", "host"),
     why="20 drifting fields: no stale gathered segment is read where med_gather is not cleared")(_drift)
CASES["bands2/band_4093"]["transports"] = ("host", "peer", "peer_nohooks")
CASES["bands2/compact_hit"]["transports"] = ("host", "peer", "peer_nohooks")
