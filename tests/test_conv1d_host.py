"""CPU tests of the CONV1D models (--model CONV1D, massiveMIMO_CSI_prediction_DNN.py:236-270): the C-ABI entry point
csi_set_model_type, the conv layers in Keras HDF5 files and SavedModel checkpoints, the weight-shape rules and the CLI.  No GPU."""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _weights(nt, hidden=(16, 8), n_out=234, seed=0, use_bn=True):
    rng = np.random.default_rng(seed)
    w = {'cnn1d_1.kernel': rng.standard_normal((7, 1, 128)).astype(np.float32),
         'cnn1d_1.bias': rng.standard_normal(128).astype(np.float32),
         'conv_bn.gamma': rng.standard_normal(128).astype(np.float32),
         'conv_bn.beta': rng.standard_normal(128).astype(np.float32),
         'conv_bn.moving_mean': rng.standard_normal(128).astype(np.float32),
         'conv_bn.moving_variance': rng.uniform(0.5, 2.0, 128).astype(np.float32)}
    fan = 64 * 320 * nt + nt
    for i, h in enumerate(hidden):
        w[f'fc_dense{i}.kernel'] = rng.standard_normal((fan, h)).astype(np.float32)
        w[f'fc_dense{i}.bias'] = rng.standard_normal(h).astype(np.float32)
        if use_bn:
            for v in ('gamma', 'beta', 'moving_mean'):
                w[f'bn{i}.{v}'] = rng.standard_normal(h).astype(np.float32)
            w[f'bn{i}.moving_variance'] = rng.uniform(0.5, 2.0, h).astype(np.float32)
        fan = h
    w['fc_regressor.kernel'] = rng.standard_normal((fan, n_out)).astype(np.float32)
    w['fc_regressor.bias'] = rng.standard_normal(n_out).astype(np.float32)
    return w


def test_header_declares_and_library_exports_csi_set_model_type(pkg):
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'csi_mamimo.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+csi_set_model_type\s*\(\s*csi_ctx\s*\*\s*ctx\s*,\s*int\s+type\s*\)\s*;', header)
    assert re.search(r'#define\s+CSI_MODEL_CONV1D\s+1', header)
    from dl_channel_estimation_mamimo_amd import _lib
    assert 'csi_set_model_type' in _lib.SYMBOLS
    lib = pkg.load_library()
    assert hasattr(lib, 'csi_set_model_type')
    names = [lib.csi_profile_kernel_name(i).decode() for i in range(lib.csi_profile_num_kernels())]
    assert 'conv_frontend' in names
    assert lib.csi_set_model_type(None, 1) != 0          # a null context is refused, no device needed


@pytest.mark.parametrize('use_bn', [True, False])
@pytest.mark.parametrize('component', ['real', 'imag'])
def test_hdf5_round_trip_in_reference_layer_order(pkg, tmp_path, component, use_bn):
    """our writer puts the conv front end where the reference's model has it (DNN.py:238-250), numbers the BatchNormalizations as
    keras does (the conv's first; the imag model, built second in the same process, continues behind the real model's), and the
    loader maps them back"""
    from dl_channel_estimation_mamimo_amd import keras_files as kf
    w = _weights(4, use_bn=use_bn)
    path = str(tmp_path / f'{component}_weights-improvement.hdf5')
    pkg.save_weight_file(path, w)
    assert kf.keras_hdf5_model_type(path) == 'CONV1D'
    names = [bytes(x).decode() for x in kf.Hdf5File(path).root.attrs['layer_names']]
    k = 0 if component == 'real' else 1
    n_bn = 1 + (2 if use_bn else 0)
    sfx = lambda base, i: base + (f'_{i}' if i else '')
    expect = [f'input_{1 + 2 * k}', 'cnn1d_1', sfx('batch_normalization', k * n_bn), sfx('average_pooling1d', k), sfx('flatten', k),
              f'input_{2 + 2 * k}', sfx('concatenate', k), 'fc_dense0']
    if use_bn:
        expect.append(sfx('batch_normalization', k * n_bn + 1))
    expect += ['drop0', 'fc_dense1']
    if use_bn:
        expect.append(sfx('batch_normalization', k * n_bn + 2))
    expect.append('fc_regressor')
    assert names == expect
    grp = kf.Hdf5File(path).root['cnn1d_1']
    assert [bytes(x).decode() for x in grp.attrs['weight_names']] == ['cnn1d_1/kernel:0', 'cnn1d_1/bias:0']
    assert grp['cnn1d_1']['kernel:0'].read().shape == (7, 1, 128)
    back = pkg.load_weight_file(path)
    assert set(back) == set(w)
    for name in w:
        np.testing.assert_array_equal(back[name].ravel(), w[name].ravel())
    from dl_channel_estimation_mamimo_amd.model import config_from_weights
    assert config_from_weights(back, 4) == dict(hidden=[16, 8], n_out=234, use_bn=use_bn)
    with pytest.raises(kf.KerasFileError, match='CONV1D'):
        kf.keras_hdf5_input_pool(path)                    # input pooling stays an FC-only question


def test_fc_file_reports_fc(pkg, tmp_path):
    from dl_channel_estimation_mamimo_amd import keras_files as kf
    w = {k: v for k, v in _weights(4).items() if not k.startswith(('cnn1d', 'conv_bn'))}
    w['fc_dense0.kernel'] = w['fc_dense0.kernel'][:320 * 4 + 4]
    path = str(tmp_path / 'real_weights-improvement.hdf5')
    pkg.save_weight_file(path, w)
    assert kf.keras_hdf5_model_type(path) == 'FC'
    assert 'batch_normalization' in [bytes(x).decode() for x in kf.Hdf5File(path).root.attrs['layer_names']]


def test_normalize_shifts_bn_numbers_behind_the_conv(pkg):
    from dl_channel_estimation_mamimo_amd.model import normalize_keras_names
    v = lambda i: np.full(3, i, np.float32)
    raw = {'cnn1d_1/kernel:0': np.zeros((7, 1, 128), np.float32), 'cnn1d_1/bias:0': np.zeros(128, np.float32)}
    for i, n in enumerate((3, 4, 5)):                      # the imag model of a 2-hidden-layer run: batch_normalization_3 .. _5
        raw[f'batch_normalization_{n}/gamma:0'] = v(i)
    out = normalize_keras_names(raw)
    assert out['conv_bn.gamma'][0] == 0 and out['bn0.gamma'][0] == 1 and out['bn1.gamma'][0] == 2
    assert 'cnn1d_1.kernel' in out and 'bn2.gamma' not in out
    fc = normalize_keras_names({f'batch_normalization_{n}/gamma:0': v(i) for i, n in enumerate((2, 3))})
    assert fc['bn0.gamma'][0] == 0 and fc['bn1.gamma'][0] == 1 and 'conv_bn.gamma' not in fc


def test_savedmodel_rank3_kernel_loads_as_cnn1d_1(pkg, tmp_path, monkeypatch):
    """the SavedModel reader: the rank-3 kernel is cnn1d_1, the BatchNormalization after it conv_bn, the Dense layers fc_dense0.. /
    fc_regressor as before"""
    from dl_channel_estimation_mamimo_amd import keras_files as kf
    w = _weights(4, hidden=(16,))
    bn = lambda p: {v: w[f'{p}.{v}'] for v in ('gamma', 'beta', 'moving_mean', 'moving_variance')}
    layers = [{'kernel': w['cnn1d_1.kernel'], 'bias': w['cnn1d_1.bias']}, bn('conv_bn'),
              {'kernel': w['fc_dense0.kernel'], 'bias': w['fc_dense0.bias']}, bn('bn0'),
              {'kernel': w['fc_regressor.kernel'], 'bias': w['fc_regressor.bias']}]
    bundle = {f'layer_with_weights-{i}/{k}/.ATTRIBUTES/VARIABLE_VALUE': v for i, lw in enumerate(layers) for k, v in lw.items()}
    (tmp_path / 'variables').mkdir()
    (tmp_path / 'variables' / 'variables.index').write_bytes(b'')
    monkeypatch.setattr(kf, 'read_tensor_bundle', lambda prefix, verify_crc=True, shapes_only=False:
                        {k: tuple(np.shape(v)) for k, v in bundle.items()} if shapes_only else bundle)
    from dl_channel_estimation_mamimo_amd import cli
    assert cli.weight_file_model_type(str(tmp_path)) == 'CONV1D'           # from the index: no shard read
    back = pkg.load_weight_file(str(tmp_path))
    assert set(back) == set(w)
    for name in w:
        np.testing.assert_array_equal(back[name], w[name])


def test_loader_refusals(pkg, tmp_path):
    from dl_channel_estimation_mamimo_amd import keras_files as kf
    w = _weights(4)
    for bad, what in ((dict(w, **{'cnn1d_1.kernel': np.zeros((5, 1, 128), np.float32)}), 'shape'),
                      ({k: v for k, v in w.items() if k != 'cnn1d_1.bias'}, 'no bias'),
                      ({k: v for k, v in w.items() if not k.startswith('conv_bn')}, 'BatchNormalization')):
        path = str(tmp_path / 'x.npz')
        np.savez(path, **bad)
        with pytest.raises(kf.KerasFileError, match='CONV1D.*' + what):
            pkg.load_weight_file(path)
    with pytest.raises(kf.KerasFileError, match='no input pooling'):
        kf.keras_layers_from_weights(w, model='CONV1D', input_pool='avg')


def test_config_from_weights_rows(pkg):
    from dl_channel_estimation_mamimo_amd import CsiError
    from dl_channel_estimation_mamimo_amd.model import config_from_weights
    w = _weights(4)
    assert config_from_weights(w, 4)['hidden'] == [16, 8]
    assert config_from_weights(w, 4, model='CONV1D')['use_bn']
    with pytest.raises(CsiError, match='CONV1D model'):
        config_from_weights({k: v for k, v in w.items() if not k.startswith(('cnn1d', 'conv_bn'))}, 4)
    with pytest.raises(CsiError):
        config_from_weights(w, 4, model='FC')


def test_engine_model_names():
    from dl_channel_estimation_mamimo_amd import CsiError
    from dl_channel_estimation_mamimo_amd.engine import model_type_name
    assert model_type_name(None) == 'FC' and model_type_name('fc') == 'FC' and model_type_name(0) == 'FC'
    assert model_type_name('CONV1D') == 'CONV1D' and model_type_name(1) == 'CONV1D'
    with pytest.raises(CsiError):
        model_type_name('CONV2D')


def test_cli_refusals(pkg, tmp_path, capsys):
    from dl_channel_estimation_mamimo_amd import cli
    with pytest.raises(SystemExit):
        cli.main(['--train', '--model', 'CONV1D', '-x', str(tmp_path / 'data.b')])
    assert 'training CONV1D models is not supported' in capsys.readouterr().out
    with pytest.raises(SystemExit):
        cli.main(['--test', '--model', 'CONV2D', '-x', str(tmp_path / 'data.b')])
    # the model type a weight file holds, and --model against it
    path = str(tmp_path / 'real_weights-improvement.safetensors')
    pkg.save_weight_file(path, _weights(4))
    h5 = str(tmp_path / 'imag_weights-improvement.hdf5')
    pkg.save_weight_file(h5, _weights(4), component='imag')
    pt = str(tmp_path / 'real_weights-improvement.pt')
    pkg.save_weight_file(pt, _weights(4))
    assert all(cli.weight_file_model_type(p) == 'CONV1D' for p in (path, h5, pt))
    fc = {k: v for k, v in _weights(4).items() if not k.startswith(('cnn1d', 'conv_bn'))}
    pkg.save_weight_file(str(tmp_path / 'fc.pt'), fc)
    assert cli.weight_file_model_type(str(tmp_path / 'fc.pt')) == 'FC'
    parse = lambda *a: cli.build_parser().parse_args(['-x', 'data.b', *a])
    loaded = [pkg.load_weight_file(p) for p in (path, h5)]
    assert cli.resolve_model_type(parse('--model', 'CONV1D'), loaded) == 'CONV1D'
    with pytest.raises(SystemExit):
        cli.resolve_model_type(parse(), loaded)
    assert 'CONV1D model' in capsys.readouterr().out
    with pytest.raises(SystemExit):
        cli.resolve_model_type(parse('--model', 'CONV1D'), [loaded[0], fc])
    assert 'disagree' in capsys.readouterr().out
