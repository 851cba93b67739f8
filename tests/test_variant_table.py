"""csrc/agx_variants.def is the one description of the kernel variants: what assistive_gym_amd.variants reads from it is what the built
library reports per variant, what the emulator libraries are compiled with, and variants.pick() chooses what the selection rule of the
emulator chose before the table existed."""
import ctypes as C
import glob
import os

import pytest

import emu_lib
from assistive_gym_amd import variants
from assistive_gym_amd.blob import DATA_DIR, ModelBlob

# kernel-name suffix per variant as bench.py looks kernels up in profiler output (its `ksuffix` dictionary), and the rag-doll variant it never runs
SUFFIX = {'feeding': '', 'feeding_l': '_fl', 'feeding_m': '_fm', 'bed_bathing': '_bb', 'bed_bathing_l': '_bbl', 'bed_bathing_m': '_bbm', 'scratch_itch': '_si',
          'scratch_itch_m': '_sim', 'dressing': '_dr', 'dressing_l': '_drl', 'dressing_m': '_drm', 'arm_manipulation': '_am', 'arm_manipulation_l': '_aml',
          'drinking': '_dk', 'drinking_l': '_dkl', 'drinking_m': '_dkm',
          'bed_settle': '_bs'}
# model -> variant, generated once from the selection expression tests/emu_lib.py carried before the table (on ndof, nrobot, NCOLL per task);
# the GPU suite asserts the same names per model from the library (feeding_l for FeedingSawyer, bed_bathing_l for the PR2, <task>_m for Stretch, ...)
MODEL_VARIANT = {
    'arm_manipulation_baxter': 'arm_manipulation_l',
    'arm_manipulation_jaco': 'arm_manipulation',
    'arm_manipulation_panda': 'arm_manipulation',
    'arm_manipulation_pr2': 'arm_manipulation_l',
    'arm_manipulation_sawyer': 'arm_manipulation',
    'bed_bathing_baxter': 'bed_bathing',
    'bed_bathing_jaco': 'bed_bathing',
    'bed_bathing_panda': 'bed_bathing',
    'bed_bathing_pr2': 'bed_bathing_l',
    'bed_bathing_sawyer': 'bed_bathing',
    'bed_bathing_stretch': 'bed_bathing_m',
    'bed_settle': 'bed_settle',
    'dressing_baxter': 'dressing',
    'dressing_jaco': 'dressing',
    'dressing_panda': 'dressing',
    'dressing_pr2': 'dressing_l',
    'dressing_sawyer': 'dressing',
    'dressing_stretch': 'dressing_m',
    'drinking_baxter': 'drinking',
    'drinking_jaco': 'drinking',
    'drinking_panda': 'drinking',
    'drinking_pr2': 'drinking_l',
    'drinking_sawyer': 'drinking',
    'drinking_stretch': 'drinking_m',
    'feeding_baxter': 'feeding_l',
    'feeding_jaco': 'feeding',
    'feeding_panda': 'feeding',
    'feeding_pr2': 'feeding_l',
    'feeding_sawyer': 'feeding_l',
    'feeding_stretch': 'feeding_m',
    'scratch_itch_baxter': 'scratch_itch',
    'scratch_itch_jaco': 'scratch_itch',
    'scratch_itch_panda': 'scratch_itch',
    'scratch_itch_pr2': 'scratch_itch',
    'scratch_itch_sawyer': 'scratch_itch',
    'scratch_itch_stretch': 'scratch_itch_m',
}


def test_table_parses():
    assert len(variants.VARIANTS) == 17
    assert {v.name: v.suffix for v in variants.VARIANTS} == SUFFIX
    assert len({v.suffix for v in variants.VARIANTS}) == 17
    # selection order: smaller limits first within a task, the rag doll behind every bed-bathing variant
    names = [v.name for v in variants.VARIANTS]
    assert names.index('bed_settle') > names.index('bed_bathing_m') > names.index('bed_bathing_l') > names.index('bed_bathing')
    assert sorted(v.name for v in variants.VARIANTS if v.manifold) == ['arm_manipulation', 'bed_bathing', 'feeding', 'scratch_itch']


class _Variant(C.Structure):      # the leading fields of struct agx_variant (csrc/agx_variant.h)
    _fields_ = [('name', C.c_char_p), ('task_kind', C.c_int)] + \
               [(k, C.c_int) for k in ('max_dof', 'max_free', 'max_block', 'max_human', 'max_coll', 'st_words', 'max_con', 'max_rows', 'lds_bytes', 'lds_solve_bytes',
                                       'scr_words', 'dbg_words', 'dbg_con', 'dbg_minv', 'dbg_hdr', 'dbg_lam', 'dbg_time', 'dbg_qdd', 'rs_narm')] + \
               [(k, C.c_void_p) for k in ('init', 'build', 'solve', 'build_mf')]


@pytest.fixture(scope='module')
def lib():
    from assistive_gym_amd.build import build
    build()
    from assistive_gym_amd import libagx
    return libagx.load()


@pytest.mark.parametrize('row', variants.VARIANTS, ids=lambda v: v.name)
def test_library_reports_the_row(lib, row):
    f = getattr(lib, 'agx_variant_' + row.name)
    f.restype = C.POINTER(_Variant)
    v = f().contents
    assert (v.name.decode(), v.task_kind, v.max_dof, v.max_free, v.max_block, v.max_coll, v.st_words) == \
           (row.name, row.task, row.max_dof, row.max_free, row.max_block, row.max_coll, row.st_words)
    assert v.max_human == variants.MAX_HUMAN
    assert bool(v.build_mf) == bool(row.manifold)


@pytest.mark.parametrize('row', variants.VARIANTS, ids=lambda v: v.name)
def test_emulator_is_compiled_with_the_row(row):
    """(No row is marked `full`: today other tests of the lean suite build the emulator library of every one of the 17 variants, so nothing is compiled
    for this test alone.  Nothing checks that; should one of those tests leave the lean suite, this one compiles the missing library itself, one g++ run.)"""
    lay = (C.c_int * 8)()
    emu_lib.lib(row.name).agx_emu_debug_layout(lay)
    assert lay[3] == row.max_dof


def test_pick_chooses_what_the_emulator_chose():
    names = sorted(os.path.basename(p)[:-len('.agxblob')] for p in glob.glob(os.path.join(DATA_DIR, '*.agxblob')))
    assert names == sorted(MODEL_VARIANT)
    n = 0
    for name in names:
        b = ModelBlob.load(name)
        for m in (b,) if name == 'bed_settle' else (b, b.coop()):      # the rag doll takes no actions: no co-op flavour
            assert variants.pick(m).name == MODEL_VARIANT[name], (name, m.is_coop)
            n += 1
    assert n == 71
