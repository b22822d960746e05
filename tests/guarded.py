"""Guard bands around device arrays (test helper, no test collects from here).

The *_device entry points of the library take raw device pointers.  A caller's array is usually a slice of a larger block (a torch
tensor inside the caching allocator's block), so what lies in front of it and behind it is live data of any value.  `Guarded` hands
an entry point such a slice of its own making: one allocation of front guard + payload + back guard, `.ptr` at the payload.  The
guards hold bit patterns that cannot reach a result unnoticed and that nothing may overwrite:

  output arrays   guards: the quiet NaN GUARD_NAN and the finite GUARD_ONE, word by word (any store shows in the NaN words; an
                  update in place - out[i] += x - hands a NaN back unchanged and shows in the finite ones); payload pre-filled with
                  a second NaN, UNWRITTEN, so that elements the call never stored can be counted afterwards
  input arrays    guards: INPUT_NAN, +3e38, INPUT_NAN, -3e38, ... word by word.  A maximum reduction built on fmaxf ignores NaN but
                  not 3e38; a product with a zero weight ignores 3e38 but not NaN; any 16-byte read outside the payload meets both.

The three NaNs differ in their payload bits on purpose.  Arithmetic hands an operand's NaN on with its payload: a kernel that read an
input guard and stored the result behind an output's payload would otherwise write exactly what the output guard already holds (seen
on the device with one NaN for both: a three-packet LS call on two-packet arrays left no trace).

Each guard is max(64 KiB, one packet of the plane = the extent of axes 1 ..) rounded up to 256 bytes, so the payload keeps the
alignment an allocation of its own has.  Everything that compares words is a pure numpy function on uint32 blocks (`make_block`,
`inspect_block`): tests/test_guarded_host.py checks those without a GPU."""
import numpy as np

GUARD_NAN = 0x7FC5A5A5          # quiet NaN, recognisable payload: every second guard word of an output
GUARD_ONE = int(np.array(1.2345679, np.float32).view(np.uint32))      # ... and the finite word between them
INPUT_NAN = 0x7FCA5A5A          # another one: every second guard word of an input
UNWRITTEN = 0x7FC3C3C3          # quiet NaN an output's payload holds before the call
BIG_POS = int(np.array(3.0e38, np.float32).view(np.uint32))
BIG_NEG = int(np.array(-3.0e38, np.float32).view(np.uint32))
MIN_GUARD_BYTES = 64 << 10


class GuardDamage(AssertionError):
    """A guard word no longer holds what was written there."""


def guard_words(shape):
    """words (4 bytes) of ONE guard of an array of this shape"""
    packet = int(np.prod(shape[1:], dtype=np.int64)) * 4
    return (max(MIN_GUARD_BYTES, packet) + 255) // 256 * 256 // 4


def guard_pattern(n, fill):
    """the n words of a guard: fill 'out' - GUARD_NAN, GUARD_ONE, ...; 'in' - INPUT_NAN, +3e38, INPUT_NAN, -3e38, ..."""
    g = np.full(n, GUARD_NAN, np.uint32)
    g[1::2] = GUARD_ONE
    if fill == 'in':
        g[0::2] = INPUT_NAN
        g[1::4] = BIG_POS
        g[3::4] = BIG_NEG
    elif fill != 'out':
        raise ValueError("fill must be 'in' or 'out', got %r" % (fill,))
    return g


def make_block(n_guard, n_payload, fill, payload=None):
    """uint32 block front guard + payload + back guard as it is uploaded; the payload is UNWRITTEN unless given (float32 or uint32 words)"""
    g = guard_pattern(n_guard, fill)
    if payload is None:
        body = np.full(n_payload, UNWRITTEN, np.uint32)
    else:
        body = np.ascontiguousarray(payload).reshape(-1).view(np.uint32)
        assert body.size == n_payload, (body.size, n_payload)
    return np.concatenate([g, body, g])


def inspect_block(block, n_guard, n_payload, fill):
    """What happened to a block since make_block: dict with
      'front' / 'back'   None, or (offset, distance, count): word offset IN THE BLOCK of the first damaged word of that guard (for the
                         front guard the damaged word NEAREST the payload is reported as well, as 'front_nearest'), its distance in
                         words from the payload edge (1 = the word that touches the payload) and the number of damaged words
      'unwritten'        word offsets IN THE PAYLOAD that still hold UNWRITTEN"""
    block = np.ascontiguousarray(block).reshape(-1).view(np.uint32)
    assert block.size == 2 * n_guard + n_payload, (block.size, n_guard, n_payload)
    want = guard_pattern(n_guard, fill)
    rep = {'front': None, 'front_nearest': None, 'back': None}
    bad = np.flatnonzero(block[:n_guard] != want)
    if bad.size:
        rep['front'] = (int(bad[0]), int(n_guard - bad[0]), int(bad.size))
        rep['front_nearest'] = (int(bad[-1]), int(n_guard - bad[-1]), int(bad.size))
    bad = np.flatnonzero(block[n_guard + n_payload:] != want)
    if bad.size:
        rep['back'] = (int(n_guard + n_payload + bad[0]), int(bad[0]) + 1, int(bad.size))
    rep['unwritten'] = np.flatnonzero(block[n_guard:n_guard + n_payload] == UNWRITTEN)
    return rep


def damage_text(rep, name=''):
    """one line per damaged guard of an inspect_block report ('' when both are intact)"""
    lines = []
    if rep['front']:
        off, dist, cnt = rep['front']
        noff, ndist, _ = rep['front_nearest']
        lines.append('%s front guard: %d damaged words, first at block offset %d (%d words = %d bytes in front of the payload), nearest at %d (%d bytes)'
                     % (name, cnt, off, dist, 4 * dist, noff, 4 * ndist))
    if rep['back']:
        off, dist, cnt = rep['back']
        lines.append('%s back guard: %d damaged words, first at block offset %d (word %d behind the payload, byte %d past its end)'
                     % (name, cnt, off, dist, 4 * (dist - 1)))
    return '\n'.join(lines)


def check_block(block, n_guard, n_payload, fill, name=''):
    """raise GuardDamage when a guard word of the block differs from what make_block wrote; returns the report otherwise"""
    rep = inspect_block(block, n_guard, n_payload, fill)
    if rep['front'] or rep['back']:
        raise GuardDamage(damage_text(rep, name))
    return rep


class Guarded:
    """A float32 device array of `shape` inside guard bands; stands in for a DeviceArray wherever only `.ptr` is read (every *_device
    method of CsiEngine).  fill 'out': an output (payload pre-filled with UNWRITTEN); fill 'in': an input, `data` uploaded at once."""

    def __init__(self, engine, shape, fill, data=None, name=''):
        self.engine, self.fill, self.name = engine, fill, name
        self.shape = tuple(int(s) for s in shape)
        self.n = int(np.prod(self.shape, dtype=np.int64))
        self.g = guard_words(self.shape)
        self.block = engine.empty((2 * self.g + self.n,))
        self.ptr = self.block.ptr + 4 * self.g
        self.nbytes = 4 * self.n
        assert self.ptr % 256 == self.block.ptr % 256
        self.sent = None
        self.block.upload(make_block(self.g, self.n, fill).view(np.float32))
        if data is not None:
            self.upload(data)

    def upload(self, host):
        """the whole payload; remembered for unchanged()"""
        host = np.ascontiguousarray(host, dtype=np.float32)
        assert host.size == self.n, (host.shape, self.shape)
        self.engine._check(self.engine._lib.csi_memcpy_h2d(self.engine._ctx, self.ptr, host.ctypes.data, host.nbytes))
        self.sent = host.reshape(self.shape).copy()
        return self

    def _whole(self):
        return self.block.download().view(np.uint32)

    def download(self):
        """the payload only"""
        return self._whole()[self.g:self.g + self.n].view(np.float32).reshape(self.shape).copy()

    def check(self):
        """GuardDamage unless both guards hold what was written"""
        check_block(self._whole(), self.g, self.n, self.fill, self.name)

    def count_unwritten(self):
        """payload words that still hold the pre-fill pattern of an output"""
        return int(inspect_block(self._whole(), self.g, self.n, self.fill)['unwritten'].size)

    def unchanged(self):
        """an input: is the payload still, bit for bit, what upload() sent?"""
        return np.array_equal(self.download().view(np.uint32), self.sent.view(np.uint32))

    def free(self):
        self.block.free()
        self.ptr = 0
