"""In-tree build of the gfx950 engine library (no JIT cache, so the .so
travels with the repository snapshot to the GPU box).

    python -m hyperopt_amd._build [--force]

The library is stamped with a hash of the sources it was compiled from
(`tpe_source_hash()`); `_lib.load()` recomputes the hash from the sources in
the tree and refuses a library built from anything else, so a stale `.so`
can never run in place of HEAD's code.
"""
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
ARCH = 'gfx950'

SOURCES = [os.path.join(HERE, 'csrc', 'tpe_engine.hip'),
           os.path.join(HERE, 'csrc', 'tpe_build.hip'),
           os.path.join(HERE, 'csrc', 'tpe_multi.hip'),
           os.path.join(HERE, 'csrc', 'tpe_window.hip'),
           os.path.join(HERE, 'csrc', 'tpe_expand.hip'),
           os.path.join(HERE, 'csrc', 'tpe_share.hip'),
           os.path.join(HERE, 'csrc', 'tpe_joint.hip'),
           os.path.join(HERE, 'csrc', 'tpe_pool.hip'),
           os.path.join(HERE, 'csrc', 'tpe_mo.hip'),
           os.path.join(HERE, 'csrc', 'tpe_mo_hv.hip'),
           os.path.join(HERE, 'csrc', 'tpe_mo_hvs.hip'),
           os.path.join(HERE, 'csrc', 'tpe_mo_hvx.hip'),
           os.path.join(HERE, 'csrc', 'tpe_mo_hvx4.hip'),
           os.path.join(HERE, 'csrc', 'tpe_mo_hvm.hip'),
           os.path.join(HERE, 'csrc', 'tpe_importance.hip'),
           os.path.join(HERE, 'csrc', 'tpe_interaction.hip'),
           os.path.join(HERE, 'csrc', 'tpe_interaction_mixed.hip'),
           os.path.join(HERE, 'csrc', 'tpe_cmodel.hip')]
DEPS = SOURCES + [os.path.join(HERE, 'csrc', 'tpe_device.h'),
                  os.path.join(HERE, 'csrc', 'tpe_ctx.h'),
                  os.path.join(HERE, 'csrc', 'tpe_mo_hv.h'),
                  os.path.join(HERE, 'csrc', 'tpe_mo_hvs.h'),
                  os.path.join(HERE, 'csrc', 'tpe_mo_hvx.h'),
                  os.path.join(HERE, 'csrc', 'tpe_mo_hvx4.h'),
                  os.path.join(HERE, 'csrc', 'tpe_mo_hvm.h'),
                  os.path.join(HERE, 'csrc', 'tpe_interaction.h'),
                  os.path.join(HERE, 'csrc', 'tpe_exp_table.h'),
                  os.path.join(REPO, 'include', 'hyperopt_tpe.h')]
TARGET = os.path.join(HERE, 'libhyperopt_tpe.so')

FLAGS = ['--offload-arch=' + ARCH, '-O3', '-std=c++17', '-fPIC', '-shared',
         '-Wall', '-Wno-unused-function', '-I' + os.path.join(REPO, 'include')]
# per-unit additions.  tpe_cmodel.hip: the compiler may not form packed-fp32
# instructions (v_pk_add/mul/fma_f32) in new units -- the existing units use
# them on purpose in one place, the fp32 screen, whose results carry an error
# bound and are re-scored in fp64 (tpe_device.h).
# The unit is fp64 throughout, so today the flag changes no instruction and no
# resource figure; it keeps a later fp32 helper from being packed silently.
# tpe_mo_hv.hip (integers and fp64 comparisons): the same.
# tpe_mo_hvs.hip (integers and fp64 comparisons): the same.
# tpe_interaction_mixed.hip (fp64 throughout): the same.
# tpe_mo_hvx.hip (fp64 throughout): the same, and no contraction into fused
# multiply-adds -- its sums are stated operation by operation, each rounded on
# its own, and posterior.mo_exclusive gives the same bits.
# tpe_mo_hvx4.hip (its four-objective counterpart): the same two.
# tpe_mo_hvm.hip (the sampled indicator): the same two -- its thresholds are an
# fp64 difference, quotient and product, each rounded on its own, and
# posterior.mo_hvm_thresholds gives the same integers.
_NO_PACKED_FP32 = ['-Xclang', '-target-feature', '-Xclang', '-packed-fp32-ops']
EXTRA_FLAGS = {'tpe_cmodel.hip': _NO_PACKED_FP32, 'tpe_mo_hv.hip': _NO_PACKED_FP32,
               'tpe_mo_hvs.hip': _NO_PACKED_FP32,
               'tpe_interaction_mixed.hip': _NO_PACKED_FP32,
               'tpe_mo_hvx.hip': _NO_PACKED_FP32 + ['-ffp-contract=off'],
               'tpe_mo_hvx4.hip': _NO_PACKED_FP32 + ['-ffp-contract=off'],
               'tpe_mo_hvm.hip': _NO_PACKED_FP32 + ['-ffp-contract=off']}


def source_hash(deps=DEPS):
    """sha256 (first 16 hex digits) over the build inputs and the flags."""
    h = hashlib.sha256()
    for d in deps:
        h.update(os.path.basename(d).encode())
        with open(d, 'rb') as f:
            h.update(f.read())
    # flags without the tree's absolute location (the GPU box unpacks it elsewhere)
    h.update(' '.join(f for f in FLAGS if not f.startswith('-I')).encode())
    for name in sorted(EXTRA_FLAGS):
        h.update((name + ' ' + ' '.join(EXTRA_FLAGS[name])).encode())
    return h.hexdigest()[:16]


def built_hash(target=TARGET):
    """The hash stamped into an existing library (None if absent/unstamped);
    read from the file's bytes, without loading it."""
    if not os.path.exists(target):
        return None
    with open(target, 'rb') as f:
        data = f.read()
    tag = b'TPE_SOURCE_HASH='
    i = data.find(tag)
    if i < 0:
        return None
    return data[i + len(tag):i + len(tag) + 16].decode('ascii', 'replace')


def build_engine(force=False, verbose=True):
    """Compile every source to an object in parallel (each carries its own
    gfx950 code object), then link the shared library."""
    import tempfile
    want = source_hash()
    if not force and built_hash(TARGET) == want:
        return TARGET
    flags = FLAGS + ['-DTPE_SOURCE_HASH="%s"' % want]
    with tempfile.TemporaryDirectory(prefix='tpe_build_') as tmp:
        objs, procs = [], []
        for src in SOURCES:
            obj = os.path.join(tmp, os.path.basename(src) + '.o')
            cmd = ([HIPCC] + [f for f in flags if f != '-shared'] + EXTRA_FLAGS.get(os.path.basename(src), [])
                   + ['-c', '-o', obj, src])
            if verbose:
                print(' '.join(cmd), flush=True)
            procs.append(subprocess.Popen(cmd))
            objs.append(obj)
        bad = [src for src, p in zip(SOURCES, procs) if p.wait() != 0]
        if bad:
            raise RuntimeError('hipcc failed on %s' % ', '.join(os.path.basename(b) for b in bad))
        cmd = [HIPCC] + flags + ['-o', TARGET] + objs
        if verbose:
            print(' '.join(cmd), flush=True)
        subprocess.check_call(cmd)
    got = built_hash(TARGET)
    if got != want:
        raise RuntimeError('built library carries hash %r, expected %r' % (got, want))
    return TARGET


def main(argv):
    build_engine(force='--force' in argv)


if __name__ == '__main__':
    main(sys.argv[1:])
