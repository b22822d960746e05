"""The sweep with a carrier frequency offset on the device (sweep --cfo EPS): a miniature run at Nt = 8, Nr = 2, two
levels, with and without the option on the same models."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_miniature_sweep_with_the_offset(pkg, tmp_path):
    from scipy.io import loadmat
    from dl_channel_estimation_mamimo_amd import sweep
    nt, nr, n_train, n_test, levels, max_eps = 8, 2, 24, 6, (0, 20), 0.05
    off, on = str(tmp_path / 'off'), str(tmp_path / 'on')
    base = ['--nTX', str(nt), '--nRX', str(nr), '--nn', '16', '--trainPkts', str(n_train), '--testPkts', str(n_test), '--snr'] + [str(s) for s in levels] + ['--quiet']
    assert sweep.main(['-d', off, '--epochs', '2', '--bs', '32'] + base) == 0                 # fits the models and saves them
    assert sweep.main(['-d', on, '--modeldir', off, '--cfo', str(max_eps)] + base) == 0
    j_off, j_on = (json.load(open(os.path.join(d, 'sweep.json'))) for d in (off, on))
    assert 'cfo' not in j_off and j_on['cfo'] == dict(max_eps=max_eps, cp_skip=0)
    new = [f + x for f in sweep.MSEO_FIELDS + sweep.MSEOC_FIELDS for x in sweep.ESTIMATORS]
    for snr, l_off, l_on in zip(levels, j_off['levels'], j_on['levels']):
        m_off, m_on = (loadmat(os.path.join(d, 'BS%d_SNR%g' % (nt, snr), 'metrics.mat')) for d in (off, on))
        old = [k for k in m_off if not k.startswith('__')]
        assert [k for k in m_on if not k.startswith('__')] == old + new
        for k in old:                                          # every old field equals a run without the option
            assert np.array_equal(m_on[k], m_off[k]), k
        for k in new:
            assert m_on[k].shape == (1, n_test) and np.isfinite(m_on[k]).all(), k
        assert all(l_on[k] == v for k, v in l_off.items() if k != 'seconds')
        print(f'{snr:g} dB: MSE_LS {l_on["LS"]["mean"]:.4e}, MSEO_LS {l_on["MSEO_LS"]["mean"]:.4e}, MSEOC_LS {l_on["MSEOC_LS"]["mean"]:.4e}, cfo_rmse '
              f'{l_on["cfo_rmse"]:.3e}, cfo_quality {l_on["cfo_quality"]:.4f}')
        assert 0.0 <= l_on['cfo_rmse'] < max_eps and 0.0 < l_on['cfo_quality'] <= 1.0 + 1e-6
    top = j_on['levels'][-1]
    assert top['MSEO_LS']['mean'] > top['MSEOC_LS']['mean']
