"""Host restatement, in fp64, of the receiver that estimates its effective channel from a precoded preamble (csi_link_sim_rx_device,
csrc/link_sim.hip.h).  Built on tests/link_ref.py and written from the definitions, not from a device run.

    n_ltf(ns) = 1, 2, 4, 4;   P = P4[0:ns, 0:n_ltf],  P4 = the 802.11 matrix, P P^T = n_ltf I
    Ypre[m][k][r] = sum_s G[k][r][s] P[s][m] + w[m][k][r],   w = the noise of symbol index n_sym + m of the data noise stream
    Ghat[k][r][s] = (1 / n_ltf) sum_m Ypre[m][k][r] P[s][m]  = G + e,  e ~ CN(0, noise_var / n_ltf)
    the data symbols pass through the true G with the draws of symbols 0 .. n_sym - 1, as in link_ref.simulate; the equaliser uses Ghat
    g_nmse = sum |Ghat - G|^2 / sum |G|^2 over (k, r, s); 0 when both sums are 0"""
import numpy as np

import link_ref as L

P4 = np.array([[1, -1, 1, 1], [1, 1, -1, 1], [1, 1, 1, -1], [-1, 1, 1, 1]], np.float64)
N_LTF = {1: 1, 2: 2, 3: 4, 4: 4}


def preamble_matrix(ns):
    """P [ns, n_ltf(ns)]"""
    return P4[:ns, :N_LTF[ns]].copy()


def estimate(G, noise_var, seed, pkt, n_sym, nr):
    """G complex [234, nr, ns] -> Ghat complex128 [234, nr, ns]: LS estimate from the n_ltf preamble symbols behind the n_sym data symbols
    of packet `pkt` in the noise stream"""
    G = np.asarray(G, np.complex128)
    P = preamble_matrix(G.shape[2])
    n_ltf = P.shape[1]
    w = np.sqrt(noise_var / 2.0) * L.noise_normals(seed, pkt, n_sym + n_ltf, nr)[n_sym:]      # [n_ltf, 234, nr]
    ypre = np.einsum('krs,sm->mkr', G, P) + w
    return np.einsum('mkr,sm->krs', ypre, P) / n_ltf


def g_nmse(Ghat, G):
    num, den = (np.abs(Ghat - G) ** 2).sum(), (np.abs(G) ** 2).sum()
    if num == 0 and den == 0:
        return 0.0
    with np.errstate(divide='ignore'):
        return float(np.float64(num) / np.float64(den))


def simulate_rx(seed, pkt, h, frf_mean, fbb, noise_var, n_sym, bps):
    """One packet in fp64.  The dict of link_ref.simulate with x, csi, cond, llr and evm_rms of the equaliser built on Ghat (cond =
    cond(Ghat)), plus Ghat, g_nmse and x_genie / csi_genie (the receiver that knows G, on the same received symbols)."""
    r = L.simulate(seed, pkt, h, frf_mean, fbb, noise_var, n_sym, bps)
    Ghat = estimate(r['G'], noise_var, seed, pkt, n_sym, h.shape[0])
    x, csi, cond = L.zero_forcing(Ghat, r['y'])
    return dict(r, x=x, csi=csi, cond=cond, llr=L.soft_bits(x, csi, noise_var, bps), evm_rms=L.evm_rms(x, bps), Ghat=Ghat,
                g_nmse=g_nmse(Ghat, r['G']), x_genie=r['x'], csi_genie=r['csi'])
