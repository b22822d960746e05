"""Beam-space bases and weights for the smoother csi_beam_* (include/csi_mamimo.h): the Nt links of every (packet, rx,
carrier) are transformed into beams, every beam is weighted by how far its power stands above the error level, and the result is
transformed back, y = A diag(w) A^H x along the antenna axis.  The module builds A in numpy fp64 and states the weight rule in
float32; the products run on the device (CsiEngine.beam_set_basis / beam_power / beam_smooth / beam_wiener)."""
import numpy as np

MAX_NT = 128


def dft_basis(nt):
    """The unitary DFT beams of a half-wavelength ULA of nt antennas, complex128 [nt, nt]:
    A[j][b] = exp(-2 pi i y_j u_b) / sqrt(nt),  y_j = (j - (nt - 1) / 2) / 2 (wavelengths),  u_b = 2 (b - nt / 2) / nt in [-1, 1).
    The sign is that of the transmit factor exp(-2 pi i y_j v_s) of the scattering generator: a path that leaves the array at the
    direction cosine v = u_b falls into beam b alone."""
    nt = int(nt)
    if not 1 <= nt <= MAX_NT:
        raise ValueError('nt %d outside 1 .. %d' % (nt, MAX_NT))
    y = (np.arange(nt, dtype=np.float64) - (nt - 1) / 2.0) / 2.0
    u = 2.0 * (np.arange(nt, dtype=np.float64) - nt / 2.0) / nt
    return np.exp(-2j * np.pi * np.outer(y, u)) / np.sqrt(nt)


def wiener_weights(power, err_var):
    """The weight rule of csi_beam_wiener[_device] in float32, the same operations in the same order: w = 1 - v / E where E > v, 0
    everywhere else (E = 0 included).  power float [..., nb], err_var float [...] (the error variance of one element of the planes).
    Returns float32 [..., nb]."""
    e = np.asarray(power, np.float32)
    v = np.asarray(err_var, np.float32)[..., None]
    with np.errstate(divide='ignore', invalid='ignore'):
        w = np.float32(1.0) - v / e
    return np.where(e > v, w, np.float32(0.0)).astype(np.float32)
