"""The kernel matrix: which compiled instantiation of the step / rollout kernels (and of the A-templated operators) each test case
is meant to launch.  A plain helper module: tests/test_kernel_matrix.py checks that the labels and the library's kernels are the
same set, tests/test_gpu_kernel_matrix.py runs every case against the oracle, scripts/kernel_coverage.py checks from a rocprofv3
trace of that run that every label was really launched.

A case's label is written by hand from the launchers (csrc/tde_api.hip, tde_launch.h, tde_step_*.hip, tde_rollout_*.hip); it is NOT derived from
a restatement of the dispatch: the trace is what confirms it."""
import re
import subprocess
from dataclasses import dataclass
from typing import Callable, Optional, Tuple

# the seven step / rollout families and the four operator families templated on A (the in-scope kernels)
STEP_ROLLOUT_FAMILIES = ("env_step_kernel", "env_step_trio_kernel", "env_step_wide_kernel", "env_rollout_kernel",
                         "env_rollout_duo_kernel", "env_rollout_trio_kernel", "env_rollout_wide_kernel")
OPERATOR_FAMILIES = ("collide_kernel", "env_reset_kernel", "first_gap_kernel", "env_post_step_kernel")
FAMILIES = STEP_ROLLOUT_FAMILIES + OPERATOR_FAMILIES

SLOTS = (1, 2, 4, 8, 16, 32, 64, 128)

# in-scope instantiations no case launches, {label: reason}; expected to stay empty
NOT_COVERED = {}

_NAME = re.compile(r"^(?:void\s+)?(?:\w+::)*(\w+)<([^<>]*)>\s*\(")


def demangle(names):
    """symbol names -> demangled names, through c++filt (names that are not mangled - rocprofv3 already demangles - come back as
    they are).  The one demangling step for library symbols and trace names alike."""
    names = [n[:-3] if n.endswith(".kd") else n for n in names]
    if not names:
        return []
    out = subprocess.run(["c++filt"], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout
    return out.splitlines()[:len(names)]


def parse(name):
    """a demangled kernel name -> (family, template args as a tuple of ints / bools), or None for a name that is not a template
    instantiation (`tde::state_obs_kernel(...)`, runtime kernels)"""
    m = _NAME.match(name.strip())
    if not m:
        return None
    args = []
    for a in m.group(2).split(","):
        a = a.strip()
        if a in ("true", "false"):
            args.append(a == "true")
        elif re.fullmatch(r"-?\d+[uUlL]*", a):
            args.append(int(re.sub(r"[uUlL]+$", "", a)))
        else:
            return None
    return m.group(1), tuple(args)


def label(family, *args):
    """the canonical text of an instantiation: env_step_kernel<64, true, false, true, 3, false>"""
    return f"{family}<{', '.join(('true' if a else 'false') if isinstance(a, bool) else str(a) for a in args)}>"


def label_of(name):
    """a demangled kernel name -> its label, or None"""
    p = parse(name)
    return None if p is None else label(p[0], *p[1])


def in_scope(lbl):
    return lbl is not None and lbl.split("<")[0] in FAMILIES


def library_labels(lib_path, workdir):
    """the labels of every in-scope instantiation in a built library (isa_audit.disassemble's kernel list)"""
    from torchdriveenv_amd import isa_audit

    _, counts = isa_audit.disassemble(lib_path, workdir)
    return {lb for lb in map(label_of, demangle(sorted(counts))) if in_scope(lb)}


# ------------------------------------------------------------------------------------------------------------------------------
# the cases

@dataclass(frozen=True)
class Case:
    world: str                          # "junctions" (synthetic_world) | "town" (large-grid synthetic_town)
    A: int
    lights: bool                        # TDE_F_TRAFFIC_LIGHTS (both worlds are signalised)
    entry: str                          # "step" | "rollout" | "collide" | "kin_collide" | "post_step" | "first_gaps"
    labels: Tuple[str, ...]             # the instantiation(s) this case is meant to launch
    B: Callable[[int], int]             # envs, as a function of the CU count
    form: Optional[str] = None          # tde_kernel_override's form ("solo" | "duo" | "trio"); None = the library's choice
    obs: bool = False                   # the state carries obs
    mag: bool = False                   # ... magnitudes
    cache: bool = True                  # ... the lookup caches
    edge: str = ""                      # a dispatch edge: the oracle runs on slices of the batch around `cuts`
    cuts: Callable[[int], Tuple[int, ...]] = lambda cu: ()

    @property
    def group(self):
        return (self.world, self.A, self.lights, self.edge)

    def id(self):
        return (f"{self.world}-A{self.A}-{'lit' if self.lights else 'dark'}-{self.entry}-{self.form or 'auto'}"
                f"{'-obs' if self.obs else ''}{'-mag' if self.mag else ''}{'' if self.cache else '-nocache'}"
                f"{'-' + self.edge if self.edge else ''}")


def _small_B(A):
    # well inside every threshold: <= 2 CUs' worth of envs at 128 slots, B*A <= 131072, one residency round of the rollouts
    return (lambda cu: min(48, 2 * cu)) if A == 128 else (lambda cu: 64)


def _om():
    return ((o, m) for o in (False, True) for m in (False, True))


def _cases():
    out = []
    for A in SLOTS:
        B = _small_B(A)
        for L in (False, True):
            J = "town" if A == 128 else "junctions"          # (no class-map form at 128 slots: the town's 128-slot scenes are full)
            # the closed-loop step, every (OBS, MAG): the one-role kernel on both worlds; the role-split kernels
            for o, m in _om():
                kw = dict(A=A, lights=L, entry="step", B=B, obs=o, mag=m)
                solo = "solo" if A in (8, 16, 32, 128) else None
                out.append(Case(world=J, labels=(label("env_step_kernel", A, L, o, False, 3, m),), form=solo, **kw))
                if A in (32, 64):
                    out.append(Case(world="town", labels=(label("env_step_kernel", A, L, o, True, 3, m),), form=solo, **kw))
                if A in (8, 16, 32):
                    out.append(Case(world=J, labels=(label("env_step_trio_kernel", A, L, o, m),), **kw))
                if A == 128:
                    out.append(Case(world=J, labels=(label("env_step_wide_kernel", L, o, m, 8),), **kw))
                    out.append(Case(world=J, labels=(label("env_step_wide_kernel", L, o, m, 4),), form="duo", **kw))
            # the persistent rollouts
            kw = dict(A=A, lights=L, entry="rollout", B=B)
            out.append(Case(world=J, labels=(label("env_rollout_kernel", A, L),), form="solo", **kw))
            if A == 128:
                out.append(Case(world=J, labels=(label("env_rollout_wide_kernel", L, 8),), **kw))
                out.append(Case(world=J, labels=(label("env_rollout_wide_kernel", L, 4),), form="duo", **kw))
            else:
                for W, big in (("junctions", False), ("town", True)):
                    out.append(Case(world=W, labels=(label("env_rollout_duo_kernel", A, L, big),), form="duo", **kw))
                    if A in (8, 16, 32):
                        out.append(Case(world=W, labels=(label("env_rollout_trio_kernel", A, L, big),), form="trio", **kw))
        # the A-templated operators (once per A, in the unlit group of the junction world / the 128-slot town)
        W = "town" if A == 128 else "junctions"
        kw = dict(world=W, A=A, lights=False, B=B)
        out.append(Case(entry="collide", labels=(label("collide_kernel", A, False),), **kw))
        out.append(Case(entry="kin_collide", labels=(label("collide_kernel", A, True),), **kw))
        out.append(Case(entry="post_step", labels=(label("env_post_step_kernel", A), label("env_reset_kernel", A)), **kw))
        out.append(Case(entry="first_gaps", labels=(label("first_gap_kernel", A),), **kw))

    # dispatch edges (csrc/tde_api.hip), both sides of each; B follows the CU count
    out += [
        # three roles up to 131072 stepping agent slots, one role above (A = 32: 4096 envs)
        Case(world="junctions", A=32, lights=False, entry="step", B=lambda cu: 4096, mag=True, edge="trio4096",
             labels=(label("env_step_trio_kernel", 32, False, False, True),), cuts=lambda cu: (4096,)),
        Case(world="junctions", A=32, lights=False, entry="step", B=lambda cu: 4097, mag=True, edge="solo4097",
             labels=(label("env_step_kernel", 32, False, False, False, 3, True),), cuts=lambda cu: (4096,)),
    ]
    for L in (False, True):
        kw = dict(world="town", A=128, lights=L, entry="step")
        out += [
            # eight wavefronts per env up to 2 x CUs envs, four above
            Case(B=lambda cu: 2 * cu, mag=True, edge="wide8", labels=(label("env_step_wide_kernel", L, False, True, 8),),
                 cuts=lambda cu: (2 * cu,), **kw),
            Case(B=lambda cu: 2 * cu + 1, mag=True, edge="wide4", labels=(label("env_step_wide_kernel", L, False, True, 4),),
                 cuts=lambda cu: (2 * cu,), **kw),
            # without the action cache: the one-role kernel at any batch size
            Case(B=lambda cu: 2 * cu, cache=False, edge="wide8", labels=(label("env_step_kernel", 128, L, False, False, 3, False),),
                 cuts=lambda cu: (2 * cu,), **kw),
            # two roles up to 4 x CUs envs, one role above
            Case(B=lambda cu: 4 * cu, obs=True, edge="duo4cu", labels=(label("env_step_wide_kernel", L, True, False, 4),),
                 cuts=lambda cu: (4 * cu,), **kw),
            Case(B=lambda cu: 4 * cu + 1, obs=True, edge="solo4cu", labels=(label("env_step_kernel", 128, L, True, False, 3, False),),
                 cuts=lambda cu: (4 * cu,), **kw),
            # the one-role kernel's three wavefronts per SIMD up to 6 x CUs envs, four above: every (OBS, MAG) of the second
            Case(B=lambda cu: 6 * cu, mag=True, edge="waves3", labels=(label("env_step_kernel", 128, L, False, False, 3, True),),
                 cuts=lambda cu: (6 * cu,), **kw),
        ]
        for o, m in _om():
            out.append(Case(B=lambda cu: 6 * cu + 1, obs=o, mag=m, edge="waves4", cuts=lambda cu: (6 * cu,),
                            labels=(label("env_step_kernel", 128, L, o, False, 4, m),), **kw))
        out.append(Case(B=lambda cu: 6 * cu + 1, cache=False, edge="waves4", cuts=lambda cu: (6 * cu,),
                        labels=(label("env_step_kernel", 128, L, False, False, 4, False),), **kw))
    # rollout chunking: one launch per residency round (8 groups of 64 slots per CU), a partial last chunk, B*A not a multiple of 64
    out += [
        Case(world="junctions", A=8, lights=False, entry="rollout", B=lambda cu: 96 * cu + 17, edge="chunks8",
             labels=(label("env_rollout_trio_kernel", 8, False, False),), cuts=lambda cu: (64 * cu, 96 * cu)),
        Case(world="town", A=32, lights=True, entry="rollout", B=lambda cu: 32 * cu + 809, edge="chunks32",
             labels=(label("env_rollout_duo_kernel", 32, True, True),), cuts=lambda cu: (16 * cu, 32 * cu)),
    ]
    return out


CASES = _cases()


def case_labels(cases=None):
    return {lb for c in (CASES if cases is None else cases) for lb in c.labels}


def groups(cases=None):
    """{(world, A, lights, edge): [cases]}, in table order"""
    out = {}
    for c in (CASES if cases is None else cases):
        out.setdefault(c.group, []).append(c)
    return out
