"""The launch plan of tests/test_gpu_instantiations.py: one recipe per k_fused instantiation the built library holds.

A key (the eight template arguments of sl3d::k_fused, 3dscan_amd/csrc/sl3d_fused_choice.h) is mapped to the contexts that can reach
it and to the launch that reaches it there:

  context   F, Gray planes per axis, parity mode or not, calibration kind, camera-table kind and a small ragged window (half of them a
            window of a larger frame).  Keys that differ only in the launch share a context: (keep, fgen, nmax, exact, rig) names it.
  launch    phase "dense" (every view densely selected) or "sparse" (every view sparsely selected, its count arrived: the gated
            forms), first view, number of views, dense planes or clouds, MASKIN (the selection handed over right before the launch).

Nothing here runs the rule: tests/test_fused_choice.py feeds every recipe's FusedShape to the rule itself
(tests/native/fused_choice_check.cpp `key`) and checks that it returns the planned key, and that the planned keys are exactly the
compiled ones.  The GPU test asserts the same key through sl3d_fused_kernel_name before and sl3d_last_fused_kernel_name after every
launch.
"""
import re
import subprocess
from dataclasses import dataclass, field

V = 8                    # views per context (>= 6; each its own capture and selection)
SMALL_LAUNCH_VIEWS = 4   # SL3D_SMALL_LAUNCH_VIEWS
_KEY_RE = re.compile(r"sl3d::k_fused<(true|false), (\d+), (true|false), (true|false), (\d), (\d), (true|false), (true|false)>")


@dataclass(frozen=True)
class Key:
    keep: bool
    nmax: int
    fgen: bool
    exact: bool
    rig: int
    cmode: int
    rcpt: bool
    early: bool

    @staticmethod
    def parse(name):
        m = _KEY_RE.fullmatch(name)
        assert m, name
        b = [v == "true" for v in m.groups()]
        g = m.groups()
        return Key(b[0], int(g[1]), b[2], b[3], int(g[4]), int(g[5]), b[6], b[7])

    @property
    def name(self):
        t = lambda v: "true" if v else "false"  # noqa: E731
        return (f"sl3d::k_fused<{t(self.keep)}, {self.nmax}, {t(self.fgen)}, {t(self.exact)}, {self.rig}, {self.cmode}, "
                f"{t(self.rcpt)}, {t(self.early)}>")


@dataclass(frozen=True)
class Launch:
    key: str
    phase: str        # "dense" / "sparse": which selections the views hold (and their counts say)
    first: int
    n: int
    clouds: bool
    maskin: bool      # the selections of [first, first + n) are handed over right before the launch (deferred)


@dataclass
class Context:
    id: str
    F: int
    nv: int
    nh: int
    keep: bool
    cal: str          # plain / projtan / projrad / k10 / k10dist (test_gpu_instantiations.py: calibration)
    cam: str          # rad / tan: the camera's distortion model (camera-table kind 1 / 2)
    skew: bool
    window: bool      # a window of a larger frame (col0 a multiple of 4, odd row0)
    seed: int
    launches: list = field(default_factory=list)

    @property
    def rig_class(self):
        """The context's rig class as sl3d_set_calibration decides it (sl3d_capi_context.cpp)."""
        if self.cal in ("k10", "k10dist"):
            return 0
        if self.cal == "plain":
            return 1
        return 3 if self.cal == "projrad" and not self.keep and self.F == 3 else 2

    def shape(self, ln):
        """The FusedShape (sl3d_fused_choice.h) of one of this context's launches, as the twelve integers of the check's `key` mode."""
        rig = self.rig_class
        proj_disp = self.cal != "plain" and self.cal != "k10" and not self.keep and rig != 3
        return (int(self.keep), self.F, self.nv, self.nh, ln.n, rig, 2 if ln.clouds else 0, int(ln.phase == "sparse"), int(ln.maskin),
                int(proj_disp), int(rig == 3), int(self.cam == "tan" and not self.keep))


def compiled_keys(lib_path):
    """Every k_fused instantiation of the built library, as rocprofv3 spells it (its host-side handles: one per kernel)."""
    nm = subprocess.run(["nm", "-C", lib_path], capture_output=True, text=True, check=True).stdout
    return sorted({line.split(" ", 2)[2].split("(")[0].removeprefix("void ") for line in nm.splitlines() if " sl3d::k_fused<" in line})


def _axes(k, i, variant):
    """Gray planes per axis for a key of nmax k.nmax; i alternates the short axis between contexts, variant between the contexts of one
    key."""
    m = k.nmax
    if k.exact:
        return m, m
    if k.keep:   # per-plane tests, bounds 8 / 12 / 16
        lo = {8: 6, 12: 9, 16: 13}[m]
        return (m, lo + i % 2) if i % 2 == 0 else (lo + 1, m)
    if m == 16:  # the per-plane-test form of the timed mode: more than 12 planes on an axis, or an axis with none
        return (13 + i % 4, 9) if variant == 0 else (7, 0)
    if m == 6:   # axes with 1..5 planes are padded up to 6
        return [(6, 3), (1 + i % 5, 6), (5, 4), (6, 5 - i % 5)][i % 4]
    return (m, m - 1) if i % 2 == 0 else (m - 2, m)


def _launches(ctx, keys):
    """The launch of each key in this context.  Small: views [0, n) with n <= 4, densely selected (not gated).  Large: views
    [1, V), densely selected (n >= 5, first_view != 0).  Gated: views [0, n) of the sparse phase, whose counts have arrived."""
    out = []
    salt = ctx.seed
    for k in keys:
        small_n = 1 + (salt + k.cmode + k.nmax) % SMALL_LAUNCH_VIEWS
        clouds, maskin = bool(k.cmode & 2), bool(k.cmode & 4)
        if k.keep or k.fgen or (k.rcpt and (k.early or k.rig == 0)):
            ln = Launch(k.name, "dense", 1, V - 1, clouds, False)
        elif not k.rcpt:
            ln = Launch(k.name, "dense", 0, small_n, clouds, maskin)
        else:   # (rcpt, not early) of a pipelined rig class: the gated form, small (MASKIN: always) or large
            n = small_n if maskin or (salt + k.nmax) % 2 == 0 else V
            ln = Launch(k.name, "sparse", 0, n, clouds, maskin)
        out.append(ln)
    return out


def _cal_variants(k):
    """(cal, cam, skew) of the contexts a key's group runs in."""
    if k.keep:
        return [({8: "plain", 12: "projtan", 16: "k10dist"}[k.nmax], "rad", False)]
    if k.rig == 0:
        if k.nmax == 16:
            return [("k10dist", "rad", False), ("projtan", "tan", False)]
        return [("k10", "rad", False), ("k10dist", "tan", False)]
    cal = {1: "plain", 2: "projtan", 3: "projrad"}[k.rig]
    # every non-MASKIN key of a pipelined class with a radial camera and with tangential terms; rig class 2 also with a skewed Kc[1]
    return [(cal, "rad", False), (cal, "tan", k.rig == 2)]


def plan(names):
    """names: the compiled k_fused names -> [Context] whose launches together name every one of them."""
    groups = {}
    for n in names:
        k = Key.parse(n)
        groups.setdefault((k.keep, k.fgen, k.nmax, k.exact, k.rig), []).append(k)
    ctxs = []
    for g, keys in sorted(groups.items()):
        keep, fgen, nmax, exact, rig = g
        keys = sorted(keys, key=lambda k: (k.cmode, k.rcpt, k.early))
        for vi, (cal, cam, skew) in enumerate(_cal_variants(keys[0])):
            for F in ((4, 5) if fgen else (3,)):
                i = len(ctxs)
                nv, nh = _axes(keys[0], i + vi, vi)
                form = ("parity" if keep else "exact" if exact else "tests" if nmax == 16 else "padded") + str(nmax)
                cid = f"F{F}-{form}-{nv}x{nh}-rig{rig}-{cal}-cam{cam}" + ("-skew" if skew else "")
                ctx = Context(cid, F, nv, nh, keep, cal, cam, skew, window=i % 2 == 1, seed=1000 + i)
                ctx.launches = _launches(ctx, [k for k in keys if not (k.cmode & 4 and cam == "tan")])
                ctxs.append(ctx)
    return ctxs


def plan_violations(ctxs, names, rule):
    """What is wrong with a plan: keys it misses or names twice in no launch, launches whose shape the rule maps elsewhere.
    rule: a function from a list of shapes to the list of key names the rule returns for them."""
    bad = []
    launches = [(c, ln) for c in ctxs for ln in c.launches]
    got = rule([c.shape(ln) for c, ln in launches])
    for (c, ln), name in zip(launches, got):
        if name != ln.key:
            bad.append(f"{c.id}: {ln} reaches {name or 'no kernel'}")
    planned = {ln.key for _, ln in launches}
    bad += [f"not planned: {n}" for n in sorted(set(names) - planned)]
    bad += [f"planned but not compiled: {n}" for n in sorted(planned - set(names))]
    ids = [c.id for c in ctxs]
    bad += [f"context id repeated: {i}" for i in sorted({i for i in ids if ids.count(i) > 1})]
    return bad
