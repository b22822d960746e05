"""Quantised CSI feedback (csi_feedback_compress_device / csi_feedback_expand_device, csrc/feedback.hip.h): the sizes,
the standard's bit pairs and the bin-centre tables of the Givens-angle report of IEEE 802.11-2016 19.3.12.3.6."""
import numpy as np

N_DATA = 234
LAYOUT_W, LAYOUT_CSI = 0, 1
MAX_NC = 4
BPHI_RANGE, BPSI_RANGE = (2, 10), (1, 8)

# (b_phi, b_psi) of the standard's codebooks: single-user feedback, codebook information 0 / 1, and multi-user feedback, 0 / 1
SU_BITS_LOW, SU_BITS_HIGH = (4, 2), (6, 4)
MU_BITS_LOW, MU_BITS_HIGH = (7, 5), (9, 7)


def n_angles(nt, nc):
    """angles of each kind (phi, psi) of an nt x nc report: sum over i < min(nc, nt - 1) of nt - 1 - i"""
    m = min(int(nc), int(nt) - 1)
    return m * (int(nt) - 1) - m * (m - 1) // 2


def n_reports(ng):
    """reported carriers of a packet: k_r = r ng, r < ceil(234 / ng)"""
    return (N_DATA + int(ng) - 1) // int(ng)


def report_bits(nt, nc, b_phi, b_psi, ng=1):
    """bits of one packet's report: n_angles codes of each kind per reported carrier (sigma travels unquantised and is not counted)"""
    return n_angles(nt, nc) * (int(b_phi) + int(b_psi)) * n_reports(ng)


def centres(b_phi, b_psi):
    """the bin centres in float64: phi = pi (2^-b_phi + k 2^(1-b_phi)), psi = pi (2^-(b_psi+2) + k 2^-(b_psi+1))"""
    phi = np.pi * (2.0 ** -b_phi + np.arange(2 ** b_phi) * 2.0 ** (1 - b_phi))
    psi = np.pi * (2.0 ** -(b_psi + 2) + np.arange(2 ** b_psi) * 2.0 ** -(b_psi + 1))
    return phi, psi


def centre_tables(b_phi, b_psi):
    """(cos phi, sin phi, cos psi, sin psi) of the bin centres, computed in double and rounded to float32: the numbers the expansion
    kernel rotates with"""
    phi, psi = centres(b_phi, b_psi)
    return tuple(t.astype(np.float32) for t in (np.cos(phi), np.sin(phi), np.cos(psi), np.sin(psi)))


def check_bits(b_phi, b_psi):
    """ValueError unless (b_phi, b_psi) is (0, 0) - continuous angles - or inside the entry's ranges"""
    b_phi, b_psi = int(b_phi), int(b_psi)
    if (b_phi, b_psi) == (0, 0):
        return
    if not (BPHI_RANGE[0] <= b_phi <= BPHI_RANGE[1] and BPSI_RANGE[0] <= b_psi <= BPSI_RANGE[1]):
        raise ValueError('feedback bits (b_phi %d, b_psi %d) outside %d .. %d / %d .. %d' % ((b_phi, b_psi) + BPHI_RANGE + BPSI_RANGE))
