"""The kernel variants (limits + task layer) of csrc/agx_variants.def, the one table the build, the library and the CPU wave emulator read."""
import collections
import os
import re

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc', 'agx_variants.def')
Variant = collections.namedtuple('Variant', 'name suffix task max_dof max_free max_block max_coll st_words arena_words scr_ent manifold')
MAX_HUMAN = 20      # csrc/agx_ctx.h, the same in every variant


def _read():
    rows = []
    for m in re.finditer(r'^AGX_VARIANT\(([^)]*)\)', open(TABLE).read(), re.M):
        f = [x.strip() for x in m.group(1).split(',')]
        assert len(f) == len(Variant._fields), m.group(0)
        rows.append(Variant(f[0], f[1], *map(int, f[2:])))
    return rows


VARIANTS = _read()      # in selection order


def defines(row):
    """the -D flags csrc/agx_kernels.hip (and the emulator's build of the same sources) is compiled with for this variant"""
    return ['-DAGX_VNAME=' + row.name, '-DAGX_KSUFFIX=' + row.suffix, '-DAGX_TASK=%d' % row.task] + \
           ['-DAGX_%s=%d' % (k.upper(), getattr(row, k)) for k in ('max_dof', 'max_free', 'max_block', 'max_coll', 'st_words', 'arena_words', 'scr_ent')] + \
           ['-DAGX_HAS_MANIFOLD=%d' % row.manifold]


def pick(blob):
    """the variant agx_create takes for a model blob: the first one with the model's task whose limits hold the model, or None"""
    for v in VARIANTS:
        if v.task == blob.task_kind and blob.ndof <= v.max_dof and blob.nfree <= v.max_free and blob.nhuman <= MAX_HUMAN and blob.h['NCOLL'] <= v.max_coll and \
                blob.state_words <= v.st_words and blob.nrobot <= v.max_block and blob.nhdof <= v.max_block:
            return v
    return None
