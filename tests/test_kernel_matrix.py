"""Every compiled instantiation of the step / rollout kernels and of the A-templated operators is the label of a case of
tests/kernel_matrix.py (which tests/test_gpu_kernel_matrix.py runs against the oracle), and every label names a kernel the library
holds.  A new instantiation without a case fails here.  Host-side: the kernel list of the built library (isa_audit.disassemble)."""
import os
import shutil
import tempfile

import pytest

from tests import kernel_matrix as km
from torchdriveenv_amd import isa_audit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "torchdriveenv_amd", "libtde_hip.so")


def test_parser_on_demangled_names():
    assert km.parse("void tde::env_step_kernel<128, false, true, false, 4, true>(tde_config, tde_world, tde_state, float const*, "
                    "float*, unsigned char*)") == ("env_step_kernel", (128, False, True, False, 4, True))
    assert km.parse("void tde::env_rollout_wide_kernel<true, 8>(tde_config, tde_world, tde_state, tde_rollout)") == \
        ("env_rollout_wide_kernel", (True, 8))
    assert km.parse("void tde::env_reset_kernel<1>(tde_config, tde_world, tde_state, unsigned char const*)") == ("env_reset_kernel", (1,))
    assert km.parse("  void tde::collide_kernel<64, true>(int, float*)") == ("collide_kernel", (64, True))
    # not template instantiations: plain kernels, the runtime's own
    assert km.parse("tde::state_obs_kernel(tde_world, tde_state, float*)") is None
    assert km.parse("__amd_rocclr_copyBuffer") is None
    assert km.parse("void f<T>(int)") is None
    assert km.label("env_step_trio_kernel", 32, True, False, True) == "env_step_trio_kernel<32, true, false, true>"
    assert km.label_of("void tde::first_gap_kernel<16>(tde_config, tde_world, unsigned int)") == "first_gap_kernel<16>"
    assert km.in_scope("first_gap_kernel<16>") and not km.in_scope("render_views_kernel<true>") and not km.in_scope(None)


@pytest.mark.skipif(shutil.which("c++filt") is None, reason="no c++filt")
def test_demangling_is_one_step_for_symbols_and_trace_names():
    mangled = "_ZN3tde15env_step_kernelILi64ELb1ELb0ELb1ELi3ELb0EEEv10tde_config9tde_world9tde_statePKfPfPh"
    want = "env_step_kernel<64, true, false, true, 3, false>"
    got = km.demangle([mangled, mangled + ".kd", "void tde::env_step_kernel<64, true, false, true, 3, false>(tde_config)",
                       "__amd_rocclr_fillBufferAligned"])
    assert [km.label_of(g) for g in got] == [want, want, want, None]


def test_case_table_is_well_formed():
    ids = [c.id() for c in km.CASES]
    assert len(set(ids)) == len(ids), "two cases with the same id"
    for cu in (80, 104, 256, 304):                 # (the table is read at the device's CU count, whatever it is)
        for key, cases in km.groups().items():
            assert len({c.B(cu) for c in cases}) == 1, f"group {key} mixes batch sizes"
            for c in cases:
                assert c.B(cu) >= 1 and all(0 < x < c.B(cu) + 1 for x in c.cuts(cu)), c.id()
    for c in km.CASES:
        assert c.labels and all(km.in_scope(lb) and km.parse(lb + "()") for lb in c.labels), c.id()
        assert c.form in (None, "solo", "duo", "trio") and c.entry in ("step", "rollout", "collide", "kin_collide", "post_step",
                                                                       "first_gaps")


def test_every_instantiation_has_a_case_and_every_label_a_kernel():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    if not os.path.exists(os.path.join(isa_audit.LLVM_BIN, "llvm-objdump")) or shutil.which("c++filt") is None:
        pytest.skip("no llvm-objdump / c++filt")
    with tempfile.TemporaryDirectory() as d:
        built = km.library_labels(LIB, d)
    # the seven step / rollout families (188 instantiations at the time of writing) and the four operator families (40)
    fams = {lb.split("<")[0] for lb in built}
    assert fams == set(km.FAMILIES), sorted(fams)
    assert len({lb for lb in built if lb.split("<")[0] in km.STEP_ROLLOUT_FAMILIES}) >= 188
    labels = km.case_labels()
    orphans = sorted(built - labels - set(km.NOT_COVERED))
    assert not orphans, f"{len(orphans)} instantiation(s) no case of tests/kernel_matrix.py launches: {orphans}"
    stale = sorted((labels | set(km.NOT_COVERED)) - built)
    assert not stale, f"label(s) that name no kernel of the library: {stale}"
    assert not (labels & set(km.NOT_COVERED)), "NOT_COVERED lists a label a case launches"
    assert all(isinstance(r, str) and r for r in km.NOT_COVERED.values())


def test_a_missing_case_names_the_orphan():
    """what the coverage test reports when the only case of an instantiation is deleted (the case table minus that case)"""
    target = km.label("env_step_kernel", 64, True, False, True, 3, False)
    owners = [c for c in km.CASES if target in c.labels]
    assert len(owners) == 1
    rest = km.case_labels([c for c in km.CASES if c is not owners[0]])
    assert target not in rest and km.case_labels() - rest == {target}
