"""What csi_load_weights leaves on the device, case by case, on the model of the HIP runtime (tests/mock_library.cpp).

Shared by tools/record_weight_prep.py, which writes tests/golden/weight_prep.json, and tests/test_weight_prep_host.py, which compares
with it.  Run as a program -

    python tests/weight_prep_cases.py <repository> <libcsi_mock.so>

- it loads every case of CASES and tries every input of REFUSALS in this one process and prints one line 'WEIGHT_PREP <json>':
    cases[id]     blobs  [[bytes, SHA-256], ...] of every model buffer in wire order, the slack behind the payload included
                  meta   SHA-256 of the WireMeta record (every leading dimension, shift, has_* flag, hs_repr_err, hs_repr_ok)
                  pins   the counter "hs_weight_pins"
                  clone  csi_clone_weights into a second context gave the same blobs and the same record
                  live   hipMalloc'ed buffers left behind after both contexts were destroyed
    refusals[id]  code, text (csi_last_error), blobs (model buffers that can still be reached: 0 = not loaded), live,
                  err_e12 (the option "hs_weight_err_e12": the split copies' error as measured up to the refusal)

Widths are no multiples of 16, 32 or 64 on purpose: every padding rule is exercised."""
import ctypes
import hashlib
import json
import sys

import numpy as np

SHAPES = {'2h': (4, (40, 24), 52), '1h': (8, (72,), 52), '3h': (4, (48, 40, 24), 20), 'wide': (4, (32, 48), 300), '256': (4, (40, 24), 256)}


def _case(shape='2h', dtype='f32', **kw):
    nt, hidden, n_out = SHAPES[shape]
    return dict(dict(nt=nt, hidden=hidden, n_out=n_out, dtype=dtype, use_bn=True, len_ltf=None, input_pool=None, model='FC', edit=None, loads=('real',)), **kw)


CASES = {f'{dtype}/{shape}': _case(shape, dtype) for dtype in ('f32', 'bf16') for shape in SHAPES}
CASES.update({
    'f32/no_bn': _case(use_bn=False), 'bf16/no_bn': _case(dtype='bf16', use_bn=False),
    'f32/nt0': _case(nt=0, len_ltf=44), 'bf16/nt0': _case(dtype='bf16', nt=0, len_ltf=44),      # the per-sample path of csi_predict_samples
    'f32/pool_max': _case(input_pool='max'), 'bf16/pool_avg': _case(dtype='bf16', input_pool='avg'),
    'f32/conv1d': _case(model='CONV1D'), 'bf16/conv1d': _case(dtype='bf16', model='CONV1D'),       # nt 4: the smallest len_ltf a context with pilots has
    'f32/outlier': _case(edit='outlier'),               # one entry of fc_dense1.kernel 2^21 above the bulk: the model is pinned
    'f32/zero_kernel': _case(edit='zero'),              # wmax == 0
    'f32/inf_kernel': _case(edit='inf'),                # the non-finite branch: error 1.0
    'f32/both': _case(loads=('real', 'imag')), 'bf16/both': _case(dtype='bf16', loads=('real', 'imag')),
    'f32/reload': _case(loads=('real', 'real')), 'f32/reload_after_pin': _case(edit='outlier_first', loads=('real', 'real')),
})

# id -> (context, what is done to the good tensors, model index, pass n = 0)
REFUSALS = {
    'missing kernel': (_case(), 'del fc_dense1.kernel', 0),
    'missing kernel over a loaded model': (_case(), 'loaded; del fc_regressor.kernel', 0),
    'missing bn': (_case(), 'del bn1.beta', 0),
    'bn length': (_case(), 'bn0.gamma 41', 0),
    'rows: CONV1D hint': (_case(), 'rows 81924', 0),
    'rows: decimated hint': (_case(), 'rows 644', 0),
    'rows: plain hint on a pooled context': (_case(input_pool='avg'), 'rows 1284', 0),
    'rows: plain hint on a CONV1D context': (_case(model='CONV1D'), 'rows 1284', 0),
    'rows: no hint': (_case(), 'rows 100', 0),
    'rows: layer 1': (_case(), 'fc_dense1.kernel 39x24', 0),
    'bias length': (_case(), 'fc_dense0.bias 39', 0),
    'missing CONV1D tensor': (_case(model='CONV1D'), 'del conv_bn.moving_mean', 0),
    'CONV1D kernel shape': (_case(model='CONV1D'), 'cnn1d_1.kernel 5x128', 0),
    'CONV1D vector length': (_case(model='CONV1D'), 'conv_bn.beta 127', 0),
    'model = 2': (_case(), '', 2),
    'n = 0': (_case(), 'n0', 0),
}


def l0_rows(case):
    len_ltf = case['len_ltf'] or 320 * case['nt']
    return (64 * len_ltf if case['model'] == 'CONV1D' else len_ltf // 2 if case['input_pool'] else len_ltf) + case['nt']


def tensors(case, synth, seed=1):
    """synth.make_weights(default_rng(seed)) for the case; a context whose layer 0 is not 321 nt wide gets a kernel of its width, a CONV1D
    context the front end's tensors, from a second generator."""
    w = synth.make_weights(np.random.default_rng(seed), case['nt'], tuple(case['hidden']), n_out=case['n_out'], use_bn=case['use_bn'])
    rng, h0 = np.random.default_rng(seed + 100), case['hidden'][0]
    if l0_rows(case) != w['fc_dense0.kernel'].shape[0]:
        lim = np.sqrt(6.0 / (l0_rows(case) + h0))
        w['fc_dense0.kernel'] = rng.uniform(-lim, lim, (l0_rows(case), h0)).astype(np.float32)
    if case['model'] == 'CONV1D':
        w['cnn1d_1.kernel'] = rng.uniform(-0.1, 0.1, (7, 128)).astype(np.float32)
        w['cnn1d_1.bias'] = (0.01 * rng.standard_normal(128)).astype(np.float32)
        w['conv_bn.gamma'] = rng.uniform(0.5, 1.5, 128).astype(np.float32)
        w['conv_bn.beta'] = (0.1 * rng.standard_normal(128)).astype(np.float32)
        w['conv_bn.moving_mean'] = (0.1 * rng.standard_normal(128)).astype(np.float32)
        w['conv_bn.moving_variance'] = rng.uniform(0.5, 1.5, 128).astype(np.float32)
    return w


def edited(w, edit):
    if edit in ('outlier', 'outlier_first'):
        k = w['fc_dense1.kernel']
        k[3, 5] = np.float32(2.0 ** 21) * np.abs(k).max()
    elif edit == 'zero':
        w['fc_dense1.kernel'][:] = 0
    elif edit == 'inf':
        w['fc_regressor.kernel'][1, 2] = np.inf
    return w


def broken(w, how):
    for step in how.split('; '):
        word = step.split()
        if not word or word[0] in ('loaded', 'n0'):
            continue
        if word[0] == 'del':
            del w[word[1]]
        elif word[0] == 'rows':
            w['fc_dense0.kernel'] = np.full((int(word[1]), w['fc_dense0.kernel'].shape[1]), 0.01, np.float32)
        else:
            w[word[0]] = np.full(tuple(int(v) for v in word[1].split('x')), 0.5, np.float32)
    return w


def main(repo, so):
    sys.path.insert(0, repo)
    import dl_channel_estimation_mamimo_amd as pkg
    from dl_channel_estimation_mamimo_amd import _lib
    _lib._SO = so
    lib = _lib.load_library()
    raw = ctypes.CDLL(so)                      # the test-only entry points of tests/mock_library.cpp
    raw.csi_mock_weight_blob.restype = ctypes.c_int64
    raw.csi_mock_weight_blob.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    raw.csi_mock_wire_meta.restype = ctypes.c_int64
    raw.csi_mock_wire_meta.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    raw.csi_mock_live_allocs.restype = ctypes.c_int64

    def engine(case):
        return pkg.CsiEngine(case['nt'], 2, hidden=tuple(case['hidden']), n_out=case['n_out'], use_bn=case['use_bn'], dtype=case['dtype'],
                             len_ltf=case['len_ltf'], input_pool=case['input_pool'], model=case['model'])

    def blobs(e):
        out = []
        while True:
            p = ctypes.c_void_p()
            n = raw.csi_mock_weight_blob(e._ctx, len(out), ctypes.byref(p))
            if n < 0:
                return out
            out.append([n, hashlib.sha256(ctypes.string_at(p, n)).hexdigest()])

    def meta(e):
        buf = ctypes.create_string_buffer(raw.csi_mock_wire_meta(e._ctx, None, 0))
        raw.csi_mock_wire_meta(e._ctx, buf, len(buf))
        return hashlib.sha256(buf.raw).hexdigest()

    engine(CASES['f32/2h']).close()            # whatever the process allocates once and keeps is allocated now
    result = {'cases': {}, 'refusals': {}}
    for cid, case in CASES.items():
        live = raw.csi_mock_live_allocs()
        e = engine(case)
        for i, model in enumerate(case['loads']):
            w = tensors(case, pkg.synth, seed=1 + i)
            first_only = case['edit'] == 'outlier_first'
            e.load_weights(model, edited(w, case['edit']) if not first_only or i == 0 else w)
            assert not lib.csi_last_error(e._ctx), lib.csi_last_error(e._ctx)      # a successful load leaves no error text
        twin = engine(case)
        twin.clone_weights_from(e)
        rec = {'blobs': blobs(e), 'meta': meta(e), 'pins': e.get_option('hs_weight_pins')}
        rec['clone'] = blobs(twin) == rec['blobs'] and meta(twin) == rec['meta']
        e.close()
        twin.close()
        rec['live'] = raw.csi_mock_live_allocs() - live
        result['cases'][cid] = rec
    for rid, (case, how, model) in REFUSALS.items():
        live = raw.csi_mock_live_allocs()
        e = engine(case)
        if how.startswith('loaded'):
            e.load_weights('real', tensors(case, pkg.synth))
        keep, arr, n = e._tensor_array(broken(tensors(case, pkg.synth), how))
        code = lib.csi_load_weights(e._ctx, model, arr, 0 if how == 'n0' else n)
        rec = {'code': code, 'text': (lib.csi_last_error(e._ctx) or b'').decode(), 'blobs': len(blobs(e)), 'err_e12': e.get_option('hs_weight_err_e12')}
        e.close()
        rec['live'] = raw.csi_mock_live_allocs() - live
        result['refusals'][rid] = rec
    print('WEIGHT_PREP ' + json.dumps(result), flush=True)


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
