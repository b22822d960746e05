"""The sweep with the symbol timing on the device (sweep --timing SPAN): a miniature run at Nt = 8, Nr = 2, two
levels, 6 packets a level, with and without the option on the same models.  At 20 dB every start is found, so the corrected capture
is the level's own packets bit for bit and MSETC_LS is MSE_LS bit for bit; the cut at the fixed start SPAN / 2 misses every packet
whose start is not 32 and stands above 10 times MSE_LS."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_miniature_sweep_with_the_timing(pkg, tmp_path):
    from scipy.io import loadmat
    from dl_channel_estimation_mamimo_amd import sweep
    nt, nr, n_train, n_test, levels, span = 8, 2, 24, 6, (0, 20), 64
    off, on = str(tmp_path / 'off'), str(tmp_path / 'on')
    base = ['--nTX', str(nt), '--nRX', str(nr), '--nn', '16', '--trainPkts', str(n_train), '--testPkts', str(n_test), '--snr'] + [str(s) for s in levels] + ['--quiet']
    assert sweep.main(['-d', off, '--epochs', '2', '--bs', '32'] + base) == 0                 # fits the models and saves them
    assert sweep.main(['-d', on, '--modeldir', off, '--timing', str(span)] + base) == 0
    j_off, j_on = (json.load(open(os.path.join(d, 'sweep.json'))) for d in (off, on))
    assert 'timing' not in j_off and j_on['timing'] == dict(span=span, rho=1.0)
    new = [f + x for f in sweep.MSET_FIELDS + sweep.MSETC_FIELDS for x in sweep.ESTIMATORS]
    for snr, l_off, l_on in zip(levels, j_off['levels'], j_on['levels']):
        m_off, m_on = (loadmat(os.path.join(d, 'BS%d_SNR%g' % (nt, snr), 'metrics.mat')) for d in (off, on))
        old = [k for k in m_off if not k.startswith('__')]
        assert [k for k in m_on if not k.startswith('__')] == old + new
        for k in old:                                          # every old field equals a run without the option
            assert np.array_equal(m_on[k], m_off[k]), k
        for k in new:
            assert m_on[k].shape == (1, n_test) and np.isfinite(m_on[k]).all(), k
        assert all(l_on[k] == v for k, v in l_off.items() if k != 'seconds')
        print(f'{snr:g} dB: MSE_LS {l_on["LS"]["mean"]:.4e}, MSET_LS {l_on["MSET_LS"]["mean"]:.4e}, MSETC_LS {l_on["MSETC_LS"]["mean"]:.4e}, timing_exact '
              f'{l_on["timing_exact"]:.3f}, timing_rmse {l_on["timing_rmse"]:.3f}, timing_quality {l_on["timing_quality"]:.4f}')
        assert 0.0 <= l_on['timing_exact'] <= 1.0 and 0.0 <= l_on['timing_rmse'] <= span and 0.0 < l_on['timing_quality'] <= 1.0 + 1e-6
    top = j_on['levels'][-1]
    m_top = loadmat(os.path.join(on, 'BS%d_SNR%g' % (nt, levels[-1]), 'metrics.mat'))
    assert top['timing_exact'] == 1.0 and top['timing_rmse'] == 0.0
    assert np.array_equal(m_top['MSETC_LS'], m_top['MSE_LS'])              # the same bits in, the same bits out
    assert top['MSET_LS']['mean'] > 10.0 * top['LS']['mean']
