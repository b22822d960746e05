"""CsiEngine: one HIP context (one GPU, one stream) holding the two regressors (real, imag),
the pilot matrix and the activation workspace.  Thin object wrapper over the C-ABI."""
import collections
import ctypes
import weakref

import numpy as np

from . import _lib
from ._lib import CsiError

N_DATA = 234     # data subcarriers, generate_maMIMO_LTF.m:98
SYM_LEN = 320    # FFT 256 + CP 64, generate_maMIMO_LTF.m:96-97


def _f32c(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


class DeviceArray:
    """float32 array in HBM owned by an engine (hipMalloc through the C-ABI)."""

    def __init__(self, engine, shape):
        self.engine = engine
        self.shape = tuple(int(s) for s in shape)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * 4
        p = ctypes.c_void_p()
        engine._check(engine._lib.csi_device_malloc(engine._ctx, ctypes.byref(p), self.nbytes))
        self.ptr = p.value or 0
        engine._arrays.add(self)          # close() frees what is still alive: an array never outlives its engine as leaked HBM

    def upload(self, host, first=0):
        """Copy `host` into rows [first, first + len(host)) along axis 0 (default: the whole array)."""
        host = _f32c(host)
        row = self.nbytes // max(self.shape[0], 1)
        assert host.nbytes % max(row, 1) == 0 and first * row + host.nbytes <= self.nbytes, (host.shape, self.shape, first)
        if first == 0 and host.nbytes != self.nbytes:
            assert host.shape[1:] == self.shape[1:], (host.shape, self.shape)
        self.engine._check(self.engine._lib.csi_memcpy_h2d(self.engine._ctx, self.ptr + first * row, host.ctypes.data, host.nbytes))
        return self

    def download(self, first=0, count=None):
        """Copy back rows [first, first+count) along axis 0 (default: everything)."""
        n0 = self.shape[0]
        count = n0 - first if count is None else count
        row = self.nbytes // max(n0, 1)
        out = np.empty((count,) + self.shape[1:], dtype=np.float32)
        self.engine._check(self.engine._lib.csi_memcpy_d2h(self.engine._ctx, out.ctypes.data,
                                                           self.ptr + first * row, count * row))
        return out

    def free(self):
        if self.ptr and self.engine._ctx:
            self.engine._lib.csi_device_free(self.engine._ctx, self.ptr)
        self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceView(DeviceArray):
    """Row `index` along axis 0 of a DeviceArray as an array of its own (shape parent.shape[1:]) that owns no memory: one time slice
    of scatter_channel_at's planes as a sounding of the forecast entries (CsiEngine.view makes it).  It keeps its parent alive; freeing
    the parent by hand, or closing the engine, ends the view: free() only forgets the address."""

    def __init__(self, parent, index):
        if not 0 <= index < parent.shape[0]:
            raise IndexError(f'view: index {index} outside 0 .. {parent.shape[0] - 1}')
        self.engine, self.parent = parent.engine, parent
        self.shape = parent.shape[1:]
        self.nbytes = parent.nbytes // parent.shape[0]
        self.ptr = parent.ptr + index * self.nbytes
        self.engine._arrays.add(self)          # close() forgets the address with the parent's memory

    def free(self):
        self.ptr = 0


HybridWeights = collections.namedtuple('HybridWeights', 'fbb idx n_atoms gain frf_mean')
LinkResult = collections.namedtuple('LinkResult', 'bit_errors evm_rms dt_snr_db n_info xeq csi llr bits')
LinkRxResult = collections.namedtuple('LinkRxResult', LinkResult._fields + ('g_nmse', 'gest'))
MuLinkResult = collections.namedtuple('MuLinkResult', 'bit_errors evm_rms sinr_db n_info g xeq csi llr bits')
FeedbackReport = collections.namedtuple('FeedbackReport', 'phi_code psi_code phi psi sigma v nc b_phi b_psi ng')


def frf_from_idx(At, idx):
    """The analog part of hybrid weights: frf[..., m, :] = At[:, idx[..., m]] ([...][ntrf][Nt], the reference's orientation);
    rows of slots an early stop left empty (index -1) are zero."""
    At = np.asarray(At)
    idx = np.asarray(idx)
    return np.where(idx[..., None] >= 0, At.T[np.maximum(idx, 0)], 0).astype(At.dtype)


class CapturedGraph:
    """Several device-pointer calls of one engine as one hipGraph (CsiEngine.capture_begin / capture_end)."""

    def __init__(self, engine, handle):
        self.engine, self.handle = engine, handle

    def launch(self):
        self.engine._check(self.engine._lib.csi_capture_launch(self.engine._ctx, self.handle))

    def free(self):
        if self.handle and self.engine._ctx:
            self.engine._lib.csi_capture_free(self.engine._ctx, self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PinnedPool:
    """Fresh numpy arrays over RECYCLED pinned host buffers.  ``take(shape, dtype)`` returns an array nobody else holds - the
    reference's wrapper returns fresh arrays (inference.py:31-32) and so does this - whose memory goes back to the pool once the
    array and every view of it are garbage-collected, so a serving loop pins its result memory once, not per call (pinning a
    gigabyte costs more than the host pass it saves).  ``alloc(nbytes)`` returns an object with the buffer protocol that frees
    its memory when it is collected (CsiEngine: csi_host_malloc behind a ctypes array with a finalizer)."""

    def __init__(self, alloc, max_idle_bytes=4 << 30):
        self._alloc, self._free, self._idle, self._max = alloc, {}, 0, int(max_idle_bytes)
        self.allocated = self.reused = 0

    def take(self, shape, dtype):
        count = int(np.prod(shape))
        n = max(count * np.dtype(dtype).itemsize, 1)
        idle = self._free.get(n)
        if idle:
            buf = idle.pop()
            self._idle -= n
            self.reused += 1
        else:
            buf = self._alloc(n)
            self.allocated += 1
        flat = np.frombuffer(buf, dtype=dtype, count=count)      # every later view has THIS array as its base: it dies last
        weakref.finalize(flat, self._give_back, n, buf)
        return flat.reshape(shape)

    def _give_back(self, n, buf):
        if self._idle + n <= self._max:                           # beyond the cap the buffer is simply dropped (and freed)
            self._free.setdefault(n, []).append(buf)
            self._idle += n

    def clear(self):
        self._free.clear()
        self._idle = 0

    @property
    def idle_bytes(self):
        return self._idle


def get_unique_id():
    """128-byte RCCL unique id (ncclGetUniqueId through the C-ABI) - create on ONE rank, hand to all."""
    lib = _lib.load_library()
    buf = ctypes.create_string_buffer(128)
    rc = lib.csi_get_unique_id(buf)
    if rc != 0:
        raise CsiError(rc, (lib.csi_last_error(None) or b'').decode())
    return buf.raw


def classify_pilot(P):
    """Which LS despread ``set_pilot(P)`` will choose (host only, no GPU needed): returns (kind, sym_src, out_row) with kind
    0 = generic real P (matrix-core despread), 1 = the Sylvester Hadamard matrix, 2 = a signed row / column permutation of it
    (e.g. the 802.11 VHT mapping matrix doubled up) - 1 and 2 take the Walsh-Hadamard kernel.  For kinds 1 / 2 the tables give
    P[j, s] = rs[j] * H[sigma(j), tau(s)] * cs[s] as sym_src[u] = tau^-1(u) | (256 if cs < 0) and out_row[r] = sigma^-1(r) | (256 if rs < 0)."""
    lib = _lib.load_library()
    P = _f32c(P)
    if P.ndim != 2 or P.shape[0] != P.shape[1]:
        raise CsiError(-1, f'P must be square, got {P.shape}')
    nt = P.shape[0]
    a, b = np.zeros(max(nt, 1), np.int32), np.zeros(max(nt, 1), np.int32)
    kind = lib.csi_pilot_classify(_fp(P), nt, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), b.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    if kind < 0:
        raise CsiError(kind, 'csi_pilot_classify: bad argument')
    return kind, (a if kind else None), (b if kind else None)


INPUT_POOL_MODES = {'max': 1, 'avg': 2}


def input_pool_name(mode):
    """None / 'none' / 0 -> None, 'max' / 1 -> 'max', 'avg' / 2 -> 'avg' (csi_set_input_pool modes)."""
    if mode is None or mode == 0 or mode == 'none':
        return None
    for name, v in INPUT_POOL_MODES.items():
        if mode == name or mode == v:
            return name
    raise CsiError(-1, f"input_pool must be None, 'max' or 'avg', got {mode!r}")


MODEL_TYPES = {'FC': 0, 'CONV1D': 1}


def model_type_name(model):
    """None / 'FC' / 0 -> 'FC', 'CONV1D' / 1 -> 'CONV1D' (csi_set_model_type types; --model of the reference)."""
    if model is None:
        return 'FC'
    for name, v in MODEL_TYPES.items():
        if (isinstance(model, str) and model.upper() == name) or (not isinstance(model, str) and model == v):
            return name
    raise CsiError(-1, f"model must be 'FC' or 'CONV1D', got {model!r}")


class CsiEngine:
    """Owns a ``csi_ctx``.  Shapes follow the reference: nt tx antennas, nr rx antennas,
    len_ltf = 320*nt samples per rx preamble, FC hidden widths ``hidden`` (--nn), n_out outputs
    (massiveMIMO_CSI_prediction_DNN.py:18,227)."""

    def __init__(self, nt, nr, hidden=(1024, 1024), n_out=N_DATA, use_bn=True, bn_eps=1e-3,
                 device=0, workspace_bytes=0, dtype='f32', len_ltf=None, input_pool=None, model='FC'):
        self._lib = _lib.load_library()
        self._ctx = None
        self.nt, self.nr = int(nt), int(nr)
        # nt == 0: single-input model without pilot input (DNN.py:180,234); only predict_samples
        self.len_ltf = SYM_LEN * self.nt if self.nt > 0 else int(len_ltf)
        self.d_in = self.len_ltf + self.nt          # width of the rows the caller hands over (raw, also for a decimated-input model)
        # decimated-input model (--decimate_max / --decimate_avg): layer 0 sees len_ltf/2 + nt inputs (csi_set_input_pool)
        self.input_pool = input_pool_name(input_pool)
        # CONV1D model (--model CONV1D): Conv1D(128, 7) + BN + AveragePooling1D + Flatten in front of layer 0, which sees 64 len_ltf + nt
        # inputs (csi_set_model_type)
        self.model = model_type_name(model)
        self.l0_in = (64 * self.len_ltf if self.model == 'CONV1D' else (self.len_ltf // 2 if self.input_pool else self.len_ltf)) + self.nt
        self.hidden = tuple(int(h) for h in hidden)
        self.n_out = int(n_out)
        self.use_bn = bool(use_bn)
        self.pilot = None
        cfg = _lib.CsiConfig()
        cfg.nt, cfg.nr, cfg.len_ltf = self.nt, self.nr, self.len_ltf
        if not 1 <= len(self.hidden) <= _lib.CSI_MAX_HIDDEN:
            raise CsiError(-1, f'between 1 and {_lib.CSI_MAX_HIDDEN} hidden layers are supported')
        cfg.n_hidden = len(self.hidden)
        for i, h in enumerate(self.hidden):
            cfg.hidden[i] = h
        cfg.n_out, cfg.use_bn, cfg.bn_eps = self.n_out, int(self.use_bn), float(bn_eps)
        cfg.dtype = {'f32': _lib.CSI_DTYPE_F32, 'bf16': _lib.CSI_DTYPE_BF16}[dtype]
        cfg.device, cfg.workspace_bytes = int(device), int(workspace_bytes)
        ctx = ctypes.c_void_p()
        rc = self._lib.csi_create(ctypes.byref(cfg), ctypes.byref(ctx))
        if rc != 0:
            raise CsiError(rc, (self._lib.csi_last_error(None) or b'').decode())
        self._ctx = ctx
        try:
            if self.input_pool:
                self._check(self._lib.csi_set_input_pool(ctx, INPUT_POOL_MODES[self.input_pool]))
            if self.model != 'FC':
                self._check(self._lib.csi_set_model_type(ctx, MODEL_TYPES[self.model]))
        except CsiError:
            self._arrays = weakref.WeakSet()
            self.close()
            raise
        self._arrays = weakref.WeakSet()
        me = weakref.ref(self)                                  # (no engine -> pool -> engine cycle: an engine is freed when its last reference goes)
        self.result_pool = PinnedPool(lambda n: me()._pinned_buffer(n))       # estimate(..., pinned_results=True)

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc):
        if rc != 0:
            raise CsiError(rc, (self._lib.csi_last_error(self._ctx) or b'').decode())

    def close(self):
        if self._ctx:
            for arr in list(getattr(self, '_arrays', ())):
                arr.free()
            if getattr(self, 'result_pool', None) is not None:
                self.result_pool.clear()                             # idle pinned buffers (those behind live arrays free themselves later)
            self._lib.csi_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        self._check(self._lib.csi_synchronize(self._ctx))

    def set_option(self, name, value):
        """Tuning knobs of csi_set_option: 'use_graph', 'force_tile', 'xcd_order', 'ls_fft_first_max', 'ls_kernel',
        'f32_engine' (-1 automatic / 0 fp32 MFMA kernels / 1 split-f16 engine), 'hs_in_shift', 'hs_act_shift', ..."""
        self._check(self._lib.csi_set_option(self._ctx, name.encode(), int(value)))

    def get_option(self, name):
        """Current value of a csi_set_option knob, or of the counters 'hs_launches' / 'hs_range_fallbacks'."""
        v = ctypes.c_int64(0)
        self._check(self._lib.csi_get_option(self._ctx, name.encode(), ctypes.byref(v)))
        return int(v.value)

    def empty(self, shape):
        return DeviceArray(self, shape)

    def view(self, array, index):
        """Row `index` along axis 0 of `array` as a DeviceView: no copy, no memory of its own."""
        return DeviceView(array, int(index))

    def to_device(self, host):
        host = _f32c(host)
        return DeviceArray(self, host.shape).upload(host)

    # ------------------------------------------------------------------ model state
    def load_weights(self, model, weights):
        """model: 0/'real' or 1/'imag'.  weights: dict keras-name -> ndarray
        (fc_dense{i}.kernel [in,out], .bias, bn{i}.gamma/beta/moving_mean/moving_variance,
        fc_regressor.kernel/.bias)."""
        idx = {'real': 0, 'imag': 1}.get(model, model)
        keep, arr = [], (_lib.CsiTensor * len(weights))()
        n = 0
        for name, val in weights.items():
            if not isinstance(val, np.ndarray):
                continue
            a = _f32c(val)
            if a.ndim == 3:                   # cnn1d_1.kernel [taps, 1, filters] as keras stores it -> [taps, filters]
                a = a.reshape(a.shape[0], a.shape[1] * a.shape[2])
            keep.append(a)
            arr[n].name = name.encode()
            arr[n].data = _fp(a)
            arr[n].rows = a.shape[0] if a.ndim == 2 else 1
            arr[n].cols = a.shape[1] if a.ndim == 2 else a.size
            n += 1
        self._check(self._lib.csi_load_weights(self._ctx, int(idx), arr, n))

    # ------------------------------------------------------------------ on-box fine-tuning (csi_train_*)
    def _tensor_array(self, weights):
        keep, arr = [], (_lib.CsiTensor * max(1, len(weights)))()
        n = 0
        for name, val in weights.items():
            if not isinstance(val, np.ndarray):
                continue
            a = _f32c(val)
            keep.append(a)
            arr[n].name = name.encode()
            arr[n].data = _fp(a)
            arr[n].rows = a.shape[0] if a.ndim == 2 else 1
            arr[n].cols = a.shape[1] if a.ndim == 2 else a.size
            n += 1
        return keep, arr, n

    def train_begin(self, model, weights=None, lr=1e-4, dropout=0.15, seed=0, beta1=0.9, beta2=0.999, eps=1e-7,
                    bn_momentum=0.99):
        """Trainer of one component model (reference: Adam(lr), --dropout, keras defaults elsewhere;
        massiveMIMO_CSI_prediction_DNN.py:16,19,272).  weights=None: Glorot-uniform initialisation."""
        idx = {'real': 0, 'imag': 1}.get(model, model)
        tc = _lib.CsiTrainConfig(lr=lr, beta1=beta1, beta2=beta2, eps=eps, bn_momentum=bn_momentum, dropout=dropout, seed=seed)
        keep, arr, n = self._tensor_array(weights or {})
        self._check(self._lib.csi_train_begin(self._ctx, int(idx), ctypes.byref(tc), arr if n else None, n))

    def train_step(self, model, x, y, noise_std=0.0):
        """One optimiser step on the rows x [B, len_ltf+nt], labels y [B, n_out]; returns the batch loss."""
        idx = {'real': 0, 'imag': 1}.get(model, model)
        x, y = _f32c(x), _f32c(y)
        if x.ndim != 2 or x.shape[1] != self.d_in or y.shape != (x.shape[0], self.n_out):
            raise CsiError(-1, f'x must be [B,{self.d_in}] and y [B,{self.n_out}], got {x.shape} / {y.shape}')
        loss = ctypes.c_float()
        self._check(self._lib.csi_train_step(self._ctx, int(idx), _fp(x), _fp(y), x.shape[0], float(noise_std), ctypes.byref(loss)))
        return float(loss.value)

    def train_backward(self, model, x, y, noise_std=0.0):
        """Loss and gradients of one batch without the parameter update (data-parallel step, part 1)."""
        idx = {'real': 0, 'imag': 1}.get(model, model)
        x, y = _f32c(x), _f32c(y)
        if x.ndim != 2 or x.shape[1] != self.d_in or y.shape != (x.shape[0], self.n_out):
            raise CsiError(-1, f'x must be [B,{self.d_in}] and y [B,{self.n_out}], got {x.shape} / {y.shape}')
        loss = ctypes.c_float()
        self._check(self._lib.csi_train_backward(self._ctx, int(idx), _fp(x), _fp(y), x.shape[0], float(noise_std), ctypes.byref(loss)))
        return float(loss.value)

    def train_grads(self, model):
        """(device pointer, element count) of the flat gradient buffer (the all-reduce operand)."""
        idx = {'real': 0, 'imag': 1}.get(model, model)
        p, n = ctypes.POINTER(ctypes.c_float)(), ctypes.c_int64()
        self._check(self._lib.csi_train_grads(self._ctx, int(idx), ctypes.byref(p), ctypes.byref(n)))
        return ctypes.cast(p, ctypes.c_void_p).value, int(n.value)

    def train_apply(self, model):
        """Adam on the (all-reduced) gradients (data-parallel step, part 2)."""
        idx = {'real': 0, 'imag': 1}.get(model, model)
        self._check(self._lib.csi_train_apply(self._ctx, int(idx)))

    def train_set_dataset(self, model, ltf_table, ltf_row, itx, y):
        """Upload a training set once (csi_train_set_dataset): ltf_table [n_rows, len_ltf] every rx preamble
        of this component once, per sample its table row, tx index and labels [N, n_out]."""
        idx = {'real': 0, 'imag': 1}.get(model, model)
        table, y = _f32c(ltf_table), _f32c(y)
        row = np.ascontiguousarray(ltf_row, dtype=np.int32)
        itx = np.ascontiguousarray(itx, dtype=np.int32)
        if table.ndim != 2 or table.shape[1] != self.len_ltf or y.shape != (row.size, self.n_out) or itx.shape != row.shape:
            raise CsiError(-1, f'dataset shapes: table [n,{self.len_ltf}], ltf_row/itx [N], y [N,{self.n_out}]')
        ip = ctypes.POINTER(ctypes.c_int32)
        self._check(self._lib.csi_train_set_dataset(self._ctx, int(idx), _fp(table), table.shape[0], row.ctypes.data_as(ip),
                                                    itx.ctypes.data_as(ip), _fp(y), row.size))

    def _train_indexed(self, model, mode, ids, noise_std):
        idx = {'real': 0, 'imag': 1}.get(model, model)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        loss = ctypes.c_float()
        self._check(self._lib.csi_train_indexed(self._ctx, int(idx), mode, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ids.size,
                                                float(noise_std), ctypes.byref(loss)))
        return float(loss.value)

    def train_step_indexed(self, model, ids, noise_std=0.0):
        """One optimiser step on the samples ``ids`` of the resident dataset."""
        return self._train_indexed(model, 0, ids, noise_std)

    def train_backward_indexed(self, model, ids, noise_std=0.0):
        return self._train_indexed(model, 1, ids, noise_std)

    def train_eval_indexed(self, model, ids):
        return self._train_indexed(model, 2, ids, 0.0)

    def train_eval(self, model, x, y):
        """mse of the current trainer parameters in inference mode (the reference's val_loss)."""
        idx = {'real': 0, 'imag': 1}.get(model, model)
        x, y = _f32c(x), _f32c(y)
        if x.ndim != 2 or x.shape[1] != self.d_in or y.shape != (x.shape[0], self.n_out):
            raise CsiError(-1, f'x must be [B,{self.d_in}] and y [B,{self.n_out}], got {x.shape} / {y.shape}')
        loss = ctypes.c_float()
        self._check(self._lib.csi_train_eval(self._ctx, int(idx), _fp(x), _fp(y), x.shape[0], ctypes.byref(loss)))
        return float(loss.value)

    def train_set_lr(self, model, lr):
        idx = {'real': 0, 'imag': 1}.get(model, model)
        self._check(self._lib.csi_train_set_lr(self._ctx, int(idx), float(lr)))

    def train_tensor_names(self):
        names = []
        for i, _ in enumerate(self.hidden):
            names += [f'fc_dense{i}.kernel', f'fc_dense{i}.bias']
            if self.use_bn:
                names += [f'bn{i}.gamma', f'bn{i}.beta', f'bn{i}.moving_mean', f'bn{i}.moving_variance']
        return names + ['fc_regressor.kernel', 'fc_regressor.bias']

    def _train_shape(self, name):
        base = name[5:] if name.startswith('grad:') else name
        widths = (self.l0_in,) + self.hidden
        if base.startswith('fc_regressor'):
            fan_in, out = self.hidden[-1], self.n_out
        else:
            i = int(''.join(ch for ch in base.split('.')[0] if ch.isdigit()))
            fan_in, out = widths[i], self.hidden[i]
        return (fan_in, out) if base.endswith('.kernel') else (out,)

    def train_get(self, model, name):
        """One trainer tensor by keras name ('grad:<name>': gradient of the last step)."""
        idx = {'real': 0, 'imag': 1}.get(model, model)
        if (name[5:] if name.startswith('grad:') else name) not in self.train_tensor_names():
            raise CsiError(-1, f"train_get: unknown tensor '{name}'")
        out = np.empty(self._train_shape(name), np.float32)
        self._check(self._lib.csi_train_get(self._ctx, int(idx), name.encode(), _fp(out), out.size))
        return out

    def train_staged_input(self, model, rows):
        """The last staged batch [rows, l0_in] as layer 0 read it - noise added, a decimated-input model's LTF pooled (test hook)."""
        idx = {'real': 0, 'imag': 1}.get(model, model)
        out = np.empty((int(rows), self.l0_in), np.float32)
        self._check(self._lib.csi_train_get(self._ctx, int(idx), b'input', _fp(out), out.size))
        return out

    def train_weights(self, model):
        return {n: self.train_get(model, n) for n in self.train_tensor_names()}

    def train_end(self, model, commit=True):
        idx = {'real': 0, 'imag': 1}.get(model, model)
        self._check(self._lib.csi_train_end(self._ctx, int(idx), int(bool(commit))))

    def set_pilot(self, P):
        """P [nt, nt], row j = pilot sequence of tx j (= dataset['P'][:, j],
        massiveMIMO_dataGenerator.py:311)."""
        P = _f32c(P)
        if P.shape != (self.nt, self.nt):
            raise CsiError(-1, f'P must be [{self.nt},{self.nt}], got {P.shape}')
        self._check(self._lib.csi_set_pilot(self._ctx, _fp(P)))
        self.pilot = P.copy()          # what this object last set (sweep.make_dataset packs it into the dataset)

    # ------------------------------------------------------------------ host-buffer calls
    def _split(self, ltf, ltf_im=None):
        if ltf_im is None:
            ltf = np.asarray(ltf)
            re, im = _f32c(ltf.real), _f32c(ltf.imag)
        else:
            re, im = _f32c(ltf), _f32c(ltf_im)
        if re.ndim != 3 or re.shape[1:] != (self.nr, self.len_ltf) or im.shape != re.shape:
            raise CsiError(-1, f'preambles must be [npkt,{self.nr},{self.len_ltf}], got {re.shape}')
        return re, im

    def _out_planes(self, out, npkt, width):
        shape = (npkt, self.nr, self.nt, width)
        if out is None:
            return np.empty(shape, dtype=np.float32), np.empty(shape, dtype=np.float32)
        o_re, o_im = out
        for o in (o_re, o_im):
            if o.dtype != np.float32 or o.shape != shape or not o.flags['C_CONTIGUOUS']:
                raise CsiError(-1, f'out planes must be C-contiguous float32 {shape}')
        return o_re, o_im

    def predict(self, ltf, ltf_im=None, out=None):
        """DNN estimate.  ltf complex [npkt,nr,len_ltf] (or two float planes).
        Returns (out_real, out_imag) float32 [npkt,nr,nt,n_out]; ``out=(o_re, o_im)`` reuses caller
        buffers (pinned ones from ``pinned_empty`` are DMA'd directly)."""
        re, im = self._split(ltf, ltf_im)
        npkt = re.shape[0]
        o_re, o_im = self._out_planes(out, npkt, self.n_out)
        self._check(self._lib.csi_predict(self._ctx, _fp(re), _fp(im), npkt, _fp(o_re), _fp(o_im)))
        return o_re, o_im

    def ls_estimate(self, ltf, ltf_im=None, out=None):
        """LS estimate, complex64 [npkt,nr,nt,234]; with ``out=(h_re, h_im)`` the two float32 planes
        are returned instead (no complex assembly on the host)."""
        re, im = self._split(ltf, ltf_im)
        npkt = re.shape[0]
        h_re, h_im = self._out_planes(out, npkt, N_DATA)
        self._check(self._lib.csi_ls_estimate(self._ctx, _fp(re), _fp(im), npkt, _fp(h_re), _fp(h_im)))
        if out is not None:
            return h_re, h_im
        h = np.empty(h_re.shape, dtype=np.complex64)
        h.real = h_re
        h.imag = h_im
        return h

    def estimate(self, ltf, dnn=True, ls=True, out=None, pinned_results=False):
        """Both estimators on the arrays of the reference's deployment wrapper (inference.py:24-32): ``ltf``
        complex128 [npkt, nr, len_ltf] in, complex64 [npkt, nr, nt, n_out] (DNN) and / or [npkt, nr, nt, 234] (LS)
        out - one upload for both, the real / imag split and the complex assembly done inside the library's
        staging copies (csi_estimate_c128).  Returns (dnn, ls); an estimator that was not asked for is None.
        ``out=(dnn_buf, ls_buf)`` reuses complex64 arrays; arrays from ``pinned_empty(shape, np.complex64)`` receive the
        downloads directly (complex values assembled on the device, no host pass on the result side; same bits).
        ``pinned_results=True`` takes the result arrays from ``self.result_pool``: fresh arrays over recycled pinned buffers.
        A complex64 ``ltf`` is NOT widened: it goes through csi_estimate_c64 (uploaded as it is - straight from the array when it
        came from ``pinned_empty(shape, np.complex64)`` - and split on the device); same bits as the complex128 call on such values."""
        c64_in = isinstance(ltf, np.ndarray) and ltf.dtype == np.complex64
        ltf = np.ascontiguousarray(ltf, dtype=np.complex64 if c64_in else np.complex128)
        if ltf.ndim != 3 or ltf.shape[1:] != (self.nr, self.len_ltf):
            raise CsiError(-1, f'preambles must be [npkt,{self.nr},{self.len_ltf}], got {ltf.shape}')
        npkt = ltf.shape[0]
        bufs = []
        for want, width, given in ((dnn, self.n_out, out[0] if out else None), (ls, N_DATA, out[1] if out else None)):
            if not want:
                bufs.append(None)
                continue
            shape = (npkt, self.nr, self.nt, width)
            if given is None:
                given = self.result_pool.take(shape, np.complex64) if pinned_results else np.empty(shape, dtype=np.complex64)
            elif given.dtype != np.complex64 or given.shape != shape or not given.flags['C_CONTIGUOUS']:
                raise CsiError(-1, f'out arrays must be C-contiguous complex64 {shape}')
            bufs.append(given)
        if bufs[0] is None and bufs[1] is None:
            raise CsiError(-1, 'estimate: nothing asked for')
        self._check((self._lib.csi_estimate_c64 if c64_in else self._lib.csi_estimate_c128)(self._ctx, ltf.ctypes.data, npkt,
                                                bufs[0].ctypes.data if bufs[0] is not None else None,
                                                bufs[1].ctypes.data if bufs[1] is not None else None))
        return bufs[0], bufs[1]

    def _pinned_buffer(self, nbytes):
        """ctypes array over ``nbytes`` of pinned host memory (csi_host_malloc), freed when the ctypes array is collected."""
        p = ctypes.c_void_p()
        self._check(self._lib.csi_host_malloc(self._ctx, ctypes.byref(p), max(int(nbytes), 1)))
        buf = (ctypes.c_char * max(int(nbytes), 1)).from_address(p.value)
        lib, addr = self._lib, p.value
        weakref.finalize(buf, lambda: lib.csi_host_free(None, ctypes.c_void_p(addr)))      # (no context: the buffer may outlive the engine)
        return buf

    def pinned_empty(self, shape, dtype=np.float32):
        """numpy array in pinned host memory (csi_host_malloc); freed with the array."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = ctypes.c_void_p()
        self._check(self._lib.csi_host_malloc(self._ctx, ctypes.byref(p), max(n, 1)))
        buf = (ctypes.c_char * max(n, 1)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
        lib, addr = self._lib, p.value
        import weakref
        # no context in the finalizer: the array may outlive the engine (csi_host_free accepts NULL for that)
        weakref.finalize(buf, lambda: lib.csi_host_free(None, ctypes.c_void_p(addr)))
        return arr

    def lmmse_estimate(self, h_ls, hvec, snr_db):
        """LMMSE smoothing (LMMSE_ce.m) of an LS estimate.  h_ls complex [npkt,nr,nt,234]; hvec
        [npkt, L] (the reference's 'h' argument); snr_db [npkt, nr].  Returns complex64."""
        h_ls = np.asarray(h_ls)
        re, im = _f32c(h_ls.real), _f32c(h_ls.imag)
        npkt = re.shape[0]
        if re.shape != (npkt, self.nr, self.nt, N_DATA):
            raise CsiError(-1, f'h_ls must be [npkt,{self.nr},{self.nt},{N_DATA}], got {re.shape}')
        hvec, snr_db = _f32c(hvec), _f32c(snr_db)
        if hvec.ndim != 2 or hvec.shape[0] != npkt or snr_db.shape != (npkt, self.nr):
            raise CsiError(-1, 'hvec must be [npkt, L] and snr_db [npkt, nr]')
        o_re, o_im = np.empty_like(re), np.empty_like(re)
        self._check(self._lib.csi_lmmse_estimate(self._ctx, _fp(re), _fp(im), npkt, _fp(hvec), hvec.shape[1], _fp(snr_db),
                                                 _fp(o_re), _fp(o_im)))
        return o_re + 1j * o_im

    def lmmse_blind(self, ltf, h_ls=None, details=False):
        """LMMSE smoothing from the packet's own statistics (csi_lmmse_blind): the noise level from the null carriers of the sounding
        symbols, the frequency correlation from the LS rows of each (packet, rx) - nothing a receiver does not have.  ltf complex
        [npkt,nr,len_ltf]; h_ls complex [npkt,nr,nt,234], or None to run the LS estimate first.  Returns complex64 [npkt,nr,nt,234];
        with ``details`` also noise_var float64 [npkt,nr] and corr complex128 [npkt,nr,234]."""
        re, im = self._split(ltf, None)
        npkt = re.shape[0]
        if h_ls is None:
            h_re, h_im = self.ls_estimate(re, im, out=self._out_planes(None, npkt, N_DATA))
        else:
            h_ls = np.asarray(h_ls)
            h_re, h_im = _f32c(h_ls.real), _f32c(h_ls.imag)
        if h_re.shape != (npkt, self.nr, self.nt, N_DATA):
            raise CsiError(-1, f'h_ls must be [{npkt},{self.nr},{self.nt},{N_DATA}], got {h_re.shape}')
        o_re, o_im = np.empty_like(h_re), np.empty_like(h_re)
        nv = np.empty((npkt, self.nr), np.float64) if details else None
        corr = np.empty((npkt, self.nr, N_DATA, 2), np.float64) if details else None
        _dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if a is not None else None
        self._check(self._lib.csi_lmmse_blind(self._ctx, _fp(re), _fp(im), _fp(h_re), _fp(h_im), npkt, _fp(o_re), _fp(o_im), _dp(nv), _dp(corr)))
        out = np.empty(o_re.shape, dtype=np.complex64)
        out.real = o_re
        out.imag = o_im
        if details:
            return out, nv, corr[..., 0] + 1j * corr[..., 1]
        return out

    # ------------------------------------------------------------------ delay-subspace smoother
    def subspace_set_basis(self, Q):
        """Basis of the subspace smoother: complex [234][r] with orthonormal columns, r = 1 .. 128 (for instance
        subspace.delay_basis(L)[0]), kept on the device in float32; a second call replaces it."""
        Q = np.asarray(Q)
        if Q.ndim != 2 or Q.shape[0] != N_DATA:
            raise CsiError(-1, f'basis must be [{N_DATA}][rank], got {Q.shape}')
        re, im = _f32c(Q.real), _f32c(Q.imag)
        self._check(self._lib.csi_subspace_set_basis(self._ctx, _fp(re), _fp(im), Q.shape[1]))
        self.subspace_rank = int(Q.shape[1])

    def subspace_smooth(self, h, weights=None):
        """y = Q diag(w) Q^H x for every row of h complex [npkt,nr,nt,234] (csi_subspace_smooth; Q from subspace_set_basis).
        weights float [npkt,nr,rank], or None for the plain projection.  Returns complex64 [npkt,nr,nt,234]."""
        h = np.asarray(h)
        re, im = _f32c(h.real), _f32c(h.imag)
        npkt = re.shape[0] if re.ndim else 0
        if re.shape != (npkt, self.nr, self.nt, N_DATA):
            raise CsiError(-1, f'h must be [npkt,{self.nr},{self.nt},{N_DATA}], got {re.shape}')
        w = None
        if weights is not None:
            w = _f32c(weights)
            rank = getattr(self, 'subspace_rank', 0)
            if w.shape != (npkt, self.nr, rank):
                raise CsiError(-1, f'weights must be [{npkt},{self.nr},{rank}], got {w.shape}')
        o_re, o_im = np.empty_like(re), np.empty_like(re)
        self._check(self._lib.csi_subspace_smooth(self._ctx, _fp(re), _fp(im), npkt, _fp(w) if w is not None else None, _fp(o_re), _fp(o_im)))
        out = np.empty(o_re.shape, dtype=np.complex64)
        out.real = o_re
        out.imag = o_im
        return out

    # ------------------------------------------------------------------ beam-space smoother across the Tx antennas
    def beam_set_basis(self, A):
        """Basis of the beam-space smoother: complex [nt][nb] with orthonormal columns, nb = 1 .. nt <= 128 (for instance
        beamspace.dft_basis(nt)), kept on the device in float32; a second call replaces it."""
        A = np.asarray(A)
        if A.ndim != 2 or A.shape[0] != self.nt:
            raise CsiError(-1, f'basis must be [{self.nt}][nb], got {A.shape}')
        re, im = _f32c(A.real), _f32c(A.imag)
        self._check(self._lib.csi_beam_set_basis(self._ctx, _fp(re), _fp(im), A.shape[1]))
        self.beam_nb = int(A.shape[1])

    def _beam_planes(self, h):
        h = np.asarray(h)
        re, im = _f32c(h.real), _f32c(h.imag)
        npkt = re.shape[0] if re.ndim else 0
        if re.shape != (npkt, self.nr, self.nt, N_DATA):
            raise CsiError(-1, f'h must be [npkt,{self.nr},{self.nt},{N_DATA}], got {re.shape}')
        return re, im, npkt

    @staticmethod
    def _c64(o_re, o_im):
        out = np.empty(o_re.shape, dtype=np.complex64)
        out.real = o_re
        out.imag = o_im
        return out

    def beam_power(self, h):
        """E[p][r][b] = mean over the 234 carriers of |sum_j conj(A[j][b]) h[p][r][j][k]|^2 (csi_beam_power_device; A from
        beam_set_basis).  h complex [npkt,nr,nt,234]; returns float32 [npkt,nr,nb]."""
        re, im, npkt = self._beam_planes(h)
        nb = getattr(self, 'beam_nb', 0)
        if npkt == 0:
            return np.empty((0, self.nr, nb), np.float32)
        d_re, d_im, d_e = self.to_device(re), self.to_device(im), self.empty((npkt, self.nr, max(nb, 1)))      # no basis: the call refuses
        try:
            self.beam_power_device(d_re, d_im, npkt, d_e)
            return d_e.download()
        finally:
            for a in (d_re, d_im, d_e):
                a.free()

    def beam_smooth(self, h, weights=None):
        """y = A diag(w) A^H x along the antenna axis of h complex [npkt,nr,nt,234] (csi_beam_smooth; A from beam_set_basis).
        weights float [npkt,nr,nb], or None for the plain projection.  Returns complex64 [npkt,nr,nt,234]."""
        re, im, npkt = self._beam_planes(h)
        w = None
        if weights is not None:
            w = _f32c(weights)
            nb = getattr(self, 'beam_nb', 0)
            if w.shape != (npkt, self.nr, nb):
                raise CsiError(-1, f'weights must be [{npkt},{self.nr},{nb}], got {w.shape}')
        o_re, o_im = np.empty_like(re), np.empty_like(re)
        self._check(self._lib.csi_beam_smooth(self._ctx, _fp(re), _fp(im), npkt, _fp(w) if w is not None else None, _fp(o_re), _fp(o_im)))
        return self._c64(o_re, o_im)

    def beam_wiener(self, h, err_var, details=False):
        """The beam-space Wiener smoother (csi_beam_wiener): beam power of every (packet, rx), w = 1 - v / E where E > v and 0 elsewhere
        (beamspace.wiener_weights), then beam_smooth with these weights.  err_var float [npkt,nr]: the error variance of one element
        of h (for an LS estimate: null_noise(ltf) / nt).  Returns complex64 [npkt,nr,nt,234]; with ``details`` also w float32
        [npkt,nr,nb]."""
        re, im, npkt = self._beam_planes(h)
        v = _f32c(err_var)
        if v.shape != (npkt, self.nr):
            raise CsiError(-1, f'err_var must be [{npkt},{self.nr}], got {v.shape}')
        o_re, o_im = np.empty_like(re), np.empty_like(re)
        w = np.empty((npkt, self.nr, getattr(self, 'beam_nb', 0)), np.float32) if details else None
        self._check(self._lib.csi_beam_wiener(self._ctx, _fp(re), _fp(im), npkt, _fp(v), _fp(o_re), _fp(o_im), _fp(w) if details else None))
        out = self._c64(o_re, o_im)
        return (out, w) if details else out

    def null_noise(self, ltf):
        """The noise level of every (packet, rx) from the null carriers of the sounding symbols (csi_null_noise_device): the statistic
        csi_lmmse_blind takes, on its own.  ltf complex [npkt,nr,len_ltf]; returns float64 [npkt,nr].  The error variance of one
        element of the LS estimate of these preambles is the result / nt."""
        re, im = self._split(ltf, None)
        npkt = re.shape[0]
        if npkt == 0:
            return np.empty((0, self.nr), np.float64)
        d_re, d_im, d_nv = self.to_device(re), self.to_device(im), self.empty((npkt, self.nr, 2))
        try:
            self.null_noise_device(d_re, d_im, npkt, d_nv)
            return d_nv.download().view(np.float64)[..., 0]
        finally:
            for a in (d_re, d_im, d_nv):
                a.free()

    # ------------------------------------------------------------------ hybrid beamforming weights
    def set_dictionary(self, At):
        """Dictionary of array responses for hybrid_weights: complex [Nt][rays] (for instance synth.steering_ula), kept on the
        device; columns are used as given.  A second call replaces it."""
        At = np.asarray(At)
        if At.ndim != 2 or At.shape[0] != self.nt:
            raise CsiError(-1, f'dictionary must be [Nt={self.nt}][rays], got {At.shape}')
        re, im = _f32c(At.real), _f32c(At.imag)
        self._check(self._lib.csi_hybrid_set_dictionary(self._ctx, _fp(re), _fp(im), At.shape[1]))
        self.dictionary = (re + 1j * im).astype(np.complex64)

    def hybrid_weights(self, h, ns=1, ntrf=None, h_eval=None, stop_tol=0.0):
        """Hybrid beamforming weights (SVD + orthogonal matching pursuit, omphybweights of the reference's
        BER_test_maMIMO_LTF.m:347-376) of a CSI tensor h complex [npkt,nr,nt,234] against the dictionary of set_dictionary.
        Returns HybridWeights(fbb complex64 [npkt,234,ns,ntrf], idx int32 [npkt,234,ntrf], n_atoms int32 [npkt,234],
        gain float32 [npkt,234], frf_mean complex64 [npkt,ntrf,nt]); the analog part is frf_from_idx(At, idx).  gain is
        |h_eval frf^T fbb^T|_F^2 per subcarrier (h_eval defaults to h); ntrf defaults to ns; stop_tol <= 0 selects 1e-5."""
        ntrf = int(ns if ntrf is None else ntrf)
        h = np.asarray(h)
        re, im = _f32c(h.real), _f32c(h.imag)
        npkt = re.shape[0] if re.ndim else 0
        if re.shape != (npkt, self.nr, self.nt, N_DATA):
            raise CsiError(-1, f'h must be [npkt,{self.nr},{self.nt},{N_DATA}], got {re.shape}')
        e_re = e_im = None
        if h_eval is not None:
            h_eval = np.asarray(h_eval)
            if h_eval.shape != h.shape:
                raise CsiError(-1, f'h_eval must have the shape of h {h.shape}, got {h_eval.shape}')
            e_re, e_im = _f32c(h_eval.real), _f32c(h_eval.imag)
        shape = (npkt, N_DATA, max(int(ns), 0), max(ntrf, 0))
        f_re, f_im = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        idx = np.full((npkt, N_DATA, max(ntrf, 0)), -1, np.int32)
        n_atoms = np.zeros((npkt, N_DATA), np.int32)
        gain = np.zeros((npkt, N_DATA), np.float32)
        m_re, m_im = np.zeros((npkt, max(ntrf, 0), self.nt), np.float32), np.zeros((npkt, max(ntrf, 0), self.nt), np.float32)
        ptr = lambda a: None if a is None else a.ctypes.data
        self._check(self._lib.csi_hybrid_weights(self._ctx, ptr(re), ptr(im), ptr(e_re), ptr(e_im), npkt, int(ns), ntrf, float(stop_tol),
                                                 ptr(f_re), ptr(f_im), ptr(idx), ptr(n_atoms), ptr(gain), ptr(m_re), ptr(m_im)))
        return HybridWeights((f_re + 1j * f_im).astype(np.complex64), idx, n_atoms, gain, (m_re + 1j * m_im).astype(np.complex64))

    def hybrid_weights_device(self, d_h_re, d_h_im, npkt, ns, ntrf, d_fbb_re, d_fbb_im, d_idx, d_n_atoms=None, d_gain=None,
                              d_frf_mean_re=None, d_frf_mean_im=None, d_eval_re=None, d_eval_im=None, stop_tol=0.0):
        """Asynchronous, on the engine's stream, over DeviceArrays: the CSI planes predict_device / ls_estimate_device /
        estimate_device wrote, unchanged.  d_idx [npkt,234,ntrf] and d_n_atoms [npkt,234] hold int32 in DeviceArrays of the
        same element size: read them with ``download().view(np.int32)``.  The optional arrays may be None."""
        ptr = lambda a: None if a is None else a.ptr
        self._check(self._lib.csi_hybrid_weights_device(self._ctx, d_h_re.ptr, d_h_im.ptr, ptr(d_eval_re), ptr(d_eval_im), int(npkt), int(ns), int(ntrf),
                                                        float(stop_tol), d_fbb_re.ptr, d_fbb_im.ptr, d_idx.ptr, ptr(d_n_atoms), ptr(d_gain),
                                                        ptr(d_frf_mean_re), ptr(d_frf_mean_im)))

    # ------------------------------------------------------------------ link simulation (csrc/link_sim.hip.h)
    def link_frame_bits(self, ns, n_sym=10, bps=2):
        """(n_info, n_coded) of one packet's codeword: n_coded = ns n_sym 234 bps, n_info = n_coded / 3 - 6."""
        n_info, n_coded = ctypes.c_int64(0), ctypes.c_int64(0)
        if self._lib.csi_link_frame_bits(int(ns), int(n_sym), int(bps), ctypes.byref(n_info), ctypes.byref(n_coded)) != 0:
            raise CsiError(-1, f'csi_link_frame_bits: ns {ns} outside 1 .. 4, n_sym {n_sym} < 1 or bps {bps} not in (2, 4)')
        return int(n_info.value), int(n_coded.value)

    def link_sim_device(self, d_h_re, d_h_im, d_fbb_re, d_fbb_im, d_frf_re, d_frf_im, d_noise_var, seed, first_pkt, npkt, ns, ntrf,
                        d_bit_errors, d_evm_rms, d_dt_snr_db, n_sym=10, bps=2, d_xeq_re=None, d_xeq_im=None, d_csi=None, d_llr=None,
                        d_bits=None):
        """Coded QAM through the true channel planes d_h ([npkt,nr,nt,234]) with the hybrid weights d_fbb ([npkt,234,ns,ntrf]) and
        d_frf ([npkt,ntrf,nt], the frf_mean planes) as hybrid_weights_device writes them, noise of variance d_noise_var[p], zero forcing,
        soft bits and Viterbi decoding (csi_link_sim_device).  Asynchronous, on the engine's stream.  d_bit_errors [npkt] holds int32
        (``download().view(np.int32)``); d_bits holds npkt * n_info bytes (``download().view(np.uint8)``); the optional arrays may be None."""
        ptr = lambda a: None if a is None else a.ptr
        self._check(self._lib.csi_link_sim_device(self._ctx, d_h_re.ptr, d_h_im.ptr, d_fbb_re.ptr, d_fbb_im.ptr, d_frf_re.ptr, d_frf_im.ptr,
                                                  d_noise_var.ptr, int(seed), int(first_pkt), int(npkt), int(ns), int(ntrf), int(n_sym), int(bps),
                                                  d_bit_errors.ptr, d_evm_rms.ptr, d_dt_snr_db.ptr, ptr(d_xeq_re), ptr(d_xeq_im), ptr(d_csi),
                                                  ptr(d_llr), ptr(d_bits)))

    def link_sim(self, h, fbb, frf_mean, noise_var, seed=0, first_pkt=0, n_sym=10, bps=2, details=False):
        """The same from numpy arrays: h complex [npkt,nr,nt,234], fbb complex [npkt,234,ns,ntrf], frf_mean complex [npkt,ntrf,nt],
        noise_var [npkt] (or a scalar).  Returns LinkResult(bit_errors int32 [npkt], evm_rms, dt_snr_db float32 [npkt], n_info, ...);
        with details=True also xeq complex64 [npkt,ns,n_sym,234], csi [npkt,ns,234], llr [npkt,n_coded] and the decoded bits uint8
        [npkt,n_info] (None otherwise)."""
        return self._link_sim_host(False, h, fbb, frf_mean, noise_var, seed, first_pkt, n_sym, bps, details)

    def _link_sim_host(self, rx, h, fbb, frf_mean, noise_var, seed, first_pkt, n_sym, bps, details):
        """link_sim (rx False) and link_sim_rx (rx True): upload, one device call, download"""
        h, fbb, frf_mean = np.asarray(h), np.asarray(fbb), np.asarray(frf_mean)
        npkt = h.shape[0] if h.ndim else 0
        if h.shape != (npkt, self.nr, self.nt, N_DATA):
            raise CsiError(-1, f'h must be [npkt,{self.nr},{self.nt},{N_DATA}], got {h.shape}')
        if fbb.ndim != 4 or fbb.shape[:2] != (npkt, N_DATA):
            raise CsiError(-1, f'fbb must be [{npkt},{N_DATA},ns,ntrf], got {fbb.shape}')
        ns, ntrf = fbb.shape[2:]
        if frf_mean.shape != (npkt, ntrf, self.nt):
            raise CsiError(-1, f'frf_mean must be [{npkt},{ntrf},{self.nt}], got {frf_mean.shape}')
        nv = np.ascontiguousarray(np.broadcast_to(np.asarray(noise_var, np.float32), (npkt,)))
        n_info, n_coded = self.link_frame_bits(ns, n_sym, bps)
        dev = [self.to_device(_f32c(a)) for a in (h.real, h.imag, fbb.real, fbb.imag, frf_mean.real, frf_mean.imag, nv)]
        outs = [self.empty((npkt,)) for _ in range(4 if rx else 3)]
        extra = [None] * 7
        if details:
            extra = [self.empty((npkt, ns, n_sym, N_DATA)), self.empty((npkt, ns, n_sym, N_DATA)), self.empty((npkt, ns, N_DATA)),
                     self.empty((npkt, n_coded)), self.empty(((npkt * n_info + 3) // 4,))]
            extra += [self.empty((npkt, N_DATA, self.nr, ns)) for _ in range(2)] if rx else [None, None]
        try:
            if rx:
                self.link_sim_rx_device(*dev, seed, first_pkt, npkt, ns, ntrf, *outs, n_sym=n_sym, bps=bps, d_xeq_re=extra[0], d_xeq_im=extra[1],
                                        d_csi=extra[2], d_llr=extra[3], d_bits=extra[4], d_gest_re=extra[5], d_gest_im=extra[6])
            else:
                self.link_sim_device(*dev, seed, first_pkt, npkt, ns, ntrf, *outs, n_sym=n_sym, bps=bps, d_xeq_re=extra[0], d_xeq_im=extra[1],
                                     d_csi=extra[2], d_llr=extra[3], d_bits=extra[4])
            self.synchronize()
            res = LinkResult(outs[0].download().view(np.int32), outs[1].download(), outs[2].download(), n_info,
                             (extra[0].download() + 1j * extra[1].download()).astype(np.complex64) if details else None,
                             extra[2].download() if details else None, extra[3].download() if details else None,
                             extra[4].download().view(np.uint8)[:npkt * n_info].reshape(npkt, n_info).copy() if details else None)
            if rx:
                res = LinkRxResult(*res, outs[3].download(),
                                   (extra[5].download() + 1j * extra[6].download()).astype(np.complex64) if details else None)
        finally:
            for a in dev + outs + extra:
                if a is not None:
                    a.free()
        return res

    def link_sim_rx_device(self, d_h_re, d_h_im, d_fbb_re, d_fbb_im, d_frf_re, d_frf_im, d_noise_var, seed, first_pkt, npkt, ns, ntrf,
                           d_bit_errors, d_evm_rms, d_dt_snr_db, d_g_nmse, n_sym=10, bps=2, d_xeq_re=None, d_xeq_im=None, d_csi=None, d_llr=None,
                           d_bits=None, d_gest_re=None, d_gest_im=None):
        """link_sim_device with a receiver that estimates the effective channel from a precoded preamble of link_preamble_symbols(ns)
        symbols and equalises with the estimate (csi_link_sim_rx_device): the same bits and the same data noise.  d_g_nmse [npkt]
        receives |Ghat - G|^2 / |G|^2 per packet; the optional pair d_gest_re / d_gest_im [npkt,234,nr,ns] the estimate itself."""
        ptr = lambda a: None if a is None else a.ptr
        self._check(self._lib.csi_link_sim_rx_device(self._ctx, d_h_re.ptr, d_h_im.ptr, d_fbb_re.ptr, d_fbb_im.ptr, d_frf_re.ptr, d_frf_im.ptr,
                                                     d_noise_var.ptr, int(seed), int(first_pkt), int(npkt), int(ns), int(ntrf), int(n_sym), int(bps),
                                                     d_bit_errors.ptr, d_evm_rms.ptr, d_dt_snr_db.ptr, ptr(d_xeq_re), ptr(d_xeq_im), ptr(d_csi),
                                                     ptr(d_llr), ptr(d_bits), d_g_nmse.ptr, ptr(d_gest_re), ptr(d_gest_im)))

    def link_preamble_symbols(self, ns):
        """Symbols of the precoded preamble of ns streams: 1, 2, 4, 4."""
        n = self._lib.csi_link_preamble_symbols(int(ns))
        if n < 0:
            raise CsiError(-1, f'csi_link_preamble_symbols: ns {ns} outside 1 .. 4')
        return int(n)

    def link_sim_rx(self, h, fbb, frf_mean, noise_var, seed=0, first_pkt=0, n_sym=10, bps=2, details=False):
        """link_sim with the estimating receiver (link_sim_rx_device).  Returns LinkRxResult: the fields of LinkResult, then g_nmse
        float32 [npkt] and, with details=True, gest complex64 [npkt,234,nr,ns] (None otherwise)."""
        return self._link_sim_host(True, h, fbb, frf_mean, noise_var, seed, first_pkt, n_sym, bps, details)

    # ------------------------------------------------------------------ multi-user downlink (csrc/mu_link.hip.h)
    @staticmethod
    def _ptr_array(arrays):
        """host array of device pointers, as the csi_mu_* entry points read it"""
        return (ctypes.c_void_p * len(arrays))(*[a.ptr if a is not None else None for a in arrays])

    def mu_precoder_device(self, d_hest_re, d_hest_im, npkt, ns, d_w_re, d_w_im, d_reg=None):
        """(Regularised) zero-forcing precoder of len(d_hest_re) users from their estimated CSI planes ([npkt,nr,nt,234] each, lists of
        DeviceArrays) for ns streams per user: d_w_re / d_w_im [npkt, U ns, nt, 234] (csi_mu_precoder_device).  d_reg [npkt] or None
        (zero forcing).  Asynchronous, on the engine's stream."""
        self._check(self._lib.csi_mu_precoder_device(self._ctx, len(d_hest_re), self._ptr_array(d_hest_re), self._ptr_array(d_hest_im), int(npkt),
                                                     int(ns), d_reg.ptr if d_reg is not None else None, d_w_re.ptr, d_w_im.ptr))

    def mu_precoder(self, h_list, ns, reg=None):
        """The same from numpy arrays: h_list = U complex arrays [npkt,nr,nt,234]; reg None, a scalar or [npkt].  Returns W complex64
        [npkt, U ns, nt, 234]."""
        h_list = [np.asarray(h) for h in h_list]
        npkt = h_list[0].shape[0] if h_list and h_list[0].ndim else 0
        for h in h_list:
            if h.shape != (npkt, self.nr, self.nt, N_DATA):
                raise CsiError(-1, f'every h must be [{npkt},{self.nr},{self.nt},{N_DATA}], got {h.shape}')
        m = len(h_list) * max(int(ns), 0)
        dev = [self.to_device(_f32c(h.real)) for h in h_list] + [self.to_device(_f32c(h.imag)) for h in h_list]
        d_reg = None if reg is None else self.to_device(np.ascontiguousarray(np.broadcast_to(np.asarray(reg, np.float32), (npkt,))))
        w = [self.empty((npkt, m, self.nt, N_DATA)) for _ in range(2)]
        try:
            self.mu_precoder_device(dev[:len(h_list)], dev[len(h_list):], npkt, ns, w[0], w[1], d_reg)
            self.synchronize()
            return (w[0].download() + 1j * w[1].download()).astype(np.complex64)
        finally:
            for a in dev + w + [d_reg]:
                if a is not None:
                    a.free()

    def mu_link_sim_device(self, d_h_re, d_h_im, d_w_re, d_w_im, d_noise_var, seed, first_pkt, npkt, ns, d_bit_errors, d_evm_rms, d_sinr_db,
                           n_sym=10, bps=2, d_g_re=None, d_g_im=None, d_xeq_re=None, d_xeq_im=None, d_csi=None, d_llr=None, d_bits=None):
        """Coded QAM for len(d_h_re) users through their TRUE planes (lists of DeviceArrays [npkt,nr,nt,234]) with the precoder planes d_w
        ([npkt, U ns, nt, 234]) and noise of variance d_noise_var[u][p] (csi_mu_link_sim_device).  Results are [U, npkt]; d_bit_errors holds
        int32, d_bits U npkt n_info bytes.  Asynchronous, on the engine's stream; the optional arrays may be None."""
        ptr = lambda a: None if a is None else a.ptr
        self._check(self._lib.csi_mu_link_sim_device(self._ctx, len(d_h_re), self._ptr_array(d_h_re), self._ptr_array(d_h_im), d_w_re.ptr, d_w_im.ptr,
                                                     d_noise_var.ptr, int(seed), int(first_pkt), int(npkt), int(ns), int(n_sym), int(bps),
                                                     d_bit_errors.ptr, d_evm_rms.ptr, d_sinr_db.ptr, ptr(d_g_re), ptr(d_g_im), ptr(d_xeq_re),
                                                     ptr(d_xeq_im), ptr(d_csi), ptr(d_llr), ptr(d_bits)))

    def mu_link_sim(self, h_list, W, noise_var, seed=0, first_pkt=0, ns=1, n_sym=10, bps=2, details=False):
        """The same from numpy arrays: h_list = U complex arrays [npkt,nr,nt,234] (the true channels), W complex [npkt, U ns, nt, 234],
        noise_var a scalar, [U] or [U, npkt].  Returns MuLinkResult(bit_errors int32, evm_rms, sinr_db float32 [U, npkt], n_info, ...); with
        details=True also g complex64 [U,npkt,ns,M,234], xeq [U,npkt,ns,n_sym,234], csi [U,npkt,ns,234], llr [U,npkt,n_coded] and the decoded
        bits uint8 [U,npkt,n_info] (None otherwise)."""
        h_list, W = [np.asarray(h) for h in h_list], np.asarray(W)
        nu = len(h_list)
        npkt = W.shape[0] if W.ndim else 0
        m = nu * int(ns)
        for h in h_list:
            if h.shape != (npkt, self.nr, self.nt, N_DATA):
                raise CsiError(-1, f'every h must be [{npkt},{self.nr},{self.nt},{N_DATA}], got {h.shape}')
        if W.shape != (npkt, m, self.nt, N_DATA):
            raise CsiError(-1, f'W must be [{npkt},{m},{self.nt},{N_DATA}], got {W.shape}')
        nv = np.asarray(noise_var, np.float32)
        nv = np.ascontiguousarray(np.broadcast_to(nv[:, None] if nv.ndim == 1 else nv, (nu, npkt)))
        n_info, n_coded = self.link_frame_bits(ns, n_sym, bps)
        dev = [self.to_device(_f32c(h.real)) for h in h_list] + [self.to_device(_f32c(h.imag)) for h in h_list]
        dev += [self.to_device(_f32c(W.real)), self.to_device(_f32c(W.imag)), self.to_device(nv)]
        outs = [self.empty((nu, npkt)) for _ in range(3)]
        extra = [None] * 7
        if details:
            extra = [self.empty((nu, npkt, ns, m, N_DATA)), self.empty((nu, npkt, ns, m, N_DATA)), self.empty((nu, npkt, ns, n_sym, N_DATA)),
                     self.empty((nu, npkt, ns, n_sym, N_DATA)), self.empty((nu, npkt, ns, N_DATA)), self.empty((nu, npkt, n_coded)),
                     self.empty(((nu * npkt * n_info + 3) // 4,))]
        try:
            self.mu_link_sim_device(dev[:nu], dev[nu:2 * nu], dev[2 * nu], dev[2 * nu + 1], dev[2 * nu + 2], seed, first_pkt, npkt, ns, *outs,
                                    n_sym=n_sym, bps=bps, d_g_re=extra[0], d_g_im=extra[1], d_xeq_re=extra[2], d_xeq_im=extra[3], d_csi=extra[4],
                                    d_llr=extra[5], d_bits=extra[6])
            self.synchronize()
            c64 = lambda re, im: (re.download() + 1j * im.download()).astype(np.complex64)
            return MuLinkResult(outs[0].download().view(np.int32), outs[1].download(), outs[2].download(), n_info,
                                c64(extra[0], extra[1]) if details else None, c64(extra[2], extra[3]) if details else None,
                                extra[4].download() if details else None, extra[5].download() if details else None,
                                extra[6].download().view(np.uint8)[:nu * npkt * n_info].reshape(nu, npkt, n_info).copy() if details else None)
        finally:
            for a in dev + outs + extra:
                if a is not None:
                    a.free()

    # ------------------------------------------------------------------ multi-user hybrid precoder (csrc/mu_hybrid.hip.h)
    def mu_hybrid_precoder_device(self, d_hest_re, d_hest_im, npkt, ns, n_rf, d_w_re, d_w_im, d_idx, d_reg=None, d_fbb_re=None, d_fbb_im=None,
                                  d_score=None):
        """Hybrid precoder of len(d_hest_re) users (lists of DeviceArrays [npkt,nr,nt,234]) with n_rf RF chains on the dictionary of
        set_dictionary: per packet n_rf beams chosen greedily by their wideband score, behind them (regularised) zero forcing on the effective
        channel per subcarrier (csi_mu_hybrid_precoder_device).  d_w_re / d_w_im [npkt, U ns, nt, 234] as mu_link_sim_device reads them; d_idx
        [npkt, n_rf] holds int32 (``download().view(np.int32)``); optional: d_reg [npkt], the pair d_fbb_re / d_fbb_im [npkt, 234, n_rf, U ns],
        d_score [npkt, U ns, rays].  Asynchronous, on the engine's stream."""
        ptr = lambda a: None if a is None else a.ptr
        self._check(self._lib.csi_mu_hybrid_precoder_device(self._ctx, len(d_hest_re), self._ptr_array(d_hest_re), self._ptr_array(d_hest_im),
                                                            int(npkt), int(ns), int(n_rf), ptr(d_reg), d_w_re.ptr, d_w_im.ptr, d_idx.ptr,
                                                            ptr(d_fbb_re), ptr(d_fbb_im), ptr(d_score)))

    def mu_hybrid_precoder(self, hests, ns, n_rf, reg=None, keep_fbb=False, keep_score=False):
        """The same from numpy arrays: hests = U complex arrays [npkt,nr,nt,234]; reg None, a scalar or [npkt].  Returns (w_re, w_im float32
        [npkt, U ns, nt, 234], idx int32 [npkt, n_rf]), then with keep_fbb the baseband part fbb complex64 [npkt, 234, n_rf, U ns] and with
        keep_score the beam scores float32 [npkt, U ns, rays]; the analog part of packet p is dictionary[:, idx[p]]."""
        hests = [np.asarray(h) for h in hests]
        npkt = hests[0].shape[0] if hests and hests[0].ndim else 0
        for h in hests:
            if h.shape != (npkt, self.nr, self.nt, N_DATA):
                raise CsiError(-1, f'every h must be [{npkt},{self.nr},{self.nt},{N_DATA}], got {h.shape}')
        nu, m, q = len(hests), len(hests) * max(int(ns), 0), max(int(n_rf), 0)
        if getattr(self, 'dictionary', None) is None:
            raise CsiError(-2, 'mu_hybrid_precoder: no dictionary set (set_dictionary)')
        rays = self.dictionary.shape[1]
        dev = [self.to_device(_f32c(h.real)) for h in hests] + [self.to_device(_f32c(h.imag)) for h in hests]
        d_reg = None if reg is None else self.to_device(np.ascontiguousarray(np.broadcast_to(np.asarray(reg, np.float32), (npkt,))))
        outs = [self.empty((npkt, m, self.nt, N_DATA)), self.empty((npkt, m, self.nt, N_DATA)), self.empty((npkt, q))]
        fbb = [self.empty((npkt, N_DATA, q, m)) for _ in range(2)] if keep_fbb else [None, None]
        score = self.empty((npkt, m, rays)) if keep_score else None
        try:
            self.mu_hybrid_precoder_device(dev[:nu], dev[nu:], npkt, ns, n_rf, outs[0], outs[1], outs[2], d_reg, fbb[0], fbb[1], score)
            self.synchronize()
            res = [outs[0].download(), outs[1].download(), outs[2].download().view(np.int32)]
            if keep_fbb:
                res.append((fbb[0].download() + 1j * fbb[1].download()).astype(np.complex64))
            if keep_score:
                res.append(score.download())
            return tuple(res)
        finally:
            for a in dev + outs + fbb + [d_reg, score]:
                if a is not None:
                    a.free()

    # ------------------------------------------------------------------ multi-user JSDM precoder (csrc/mu_jsdm.hip.h)
    JSDM_PGP, JSDM_UNIT_MODULUS = 1, 2

    def mu_covariance_device(self, d_hest_re, d_hest_im, npkt, d_cov_re, d_cov_im):
        """Transmit covariances of len(d_hest_re) users (lists of DeviceArrays [npkt,nr,nt,234]) over the carriers and all receive antennas
        into d_cov_re / d_cov_im [npkt, U, nt, nt] (csi_mu_covariance_device).  Asynchronous, on the engine's stream."""
        self._check(self._lib.csi_mu_covariance_device(self._ctx, len(d_hest_re), self._ptr_array(d_hest_re), self._ptr_array(d_hest_im), int(npkt),
                                                       d_cov_re.ptr, d_cov_im.ptr))

    def mu_covariance(self, hests):
        """The same from numpy arrays: hests = U complex arrays [npkt,nr,nt,234] -> complex64 [npkt, U, nt, nt]."""
        hests = [np.asarray(h) for h in hests]
        npkt = hests[0].shape[0] if hests and hests[0].ndim else 0
        for h in hests:
            if h.shape != (npkt, self.nr, self.nt, N_DATA):
                raise CsiError(-1, f'every h must be [{npkt},{self.nr},{self.nt},{N_DATA}], got {h.shape}')
        nu = len(hests)
        dev = [self.to_device(_f32c(h.real)) for h in hests] + [self.to_device(_f32c(h.imag)) for h in hests]
        outs = [self.empty((npkt, nu, self.nt, self.nt)) for _ in range(2)]
        try:
            self.mu_covariance_device(dev[:nu], dev[nu:], npkt, outs[0], outs[1])
            self.synchronize()
            return (outs[0].download() + 1j * outs[1].download()).astype(np.complex64)
        finally:
            for a in dev + outs:
                a.free()

    def mu_jsdm_precoder_device(self, d_hest_re, d_hest_im, npkt, ns, r_star, n_beams, d_w_re, d_w_im, groups=None, rank_tol=0.05, flags=1,
                                d_reg=None, d_cov_re=None, d_cov_im=None, d_frf_re=None, d_frf_im=None, d_fbb_re=None, d_fbb_im=None, d_eig=None,
                                d_ustar_re=None, d_ustar_im=None, d_rank=None):
        """JSDM precoder of len(d_hest_re) users (lists of DeviceArrays [npkt,nr,nt,234]): per packet the analog matrix from the eigenvectors
        of the group covariances after nulling r_star directions of every other group, n_beams RF chains per group, and behind it
        (regularised) zero forcing on the effective channel per subcarrier (csi_mu_jsdm_precoder_device).  groups: None (every user its own
        group) or U ints 0 .. G-1; flags: JSDM_PGP (per-group processing) | JSDM_UNIT_MODULUS.  d_w_re / d_w_im [npkt, U ns, nt, 234] as
        mu_link_sim_device reads them; optional: d_reg [npkt], the pair d_cov_* [npkt, U, nt, nt] IN (replaces the covariance step), the
        pairs d_frf_* [npkt, nt, G n_beams], d_fbb_* [npkt, 234, G n_beams, U ns], d_eig [npkt, G, nt], the pair d_ustar_* [npkt, G, nt,
        r_star], d_rank [npkt, G, 2] holding int32 (``download().view(np.int32)``).  Asynchronous, on the engine's stream."""
        ptr = lambda a: None if a is None else a.ptr
        grp = None if groups is None else (ctypes.c_int32 * len(groups))(*[int(g) for g in groups])
        self._check(self._lib.csi_mu_jsdm_precoder_device(self._ctx, len(d_hest_re), self._ptr_array(d_hest_re), self._ptr_array(d_hest_im),
                                                          int(npkt), int(ns), grp, int(r_star), int(n_beams), float(rank_tol), int(flags),
                                                          ptr(d_reg), ptr(d_cov_re), ptr(d_cov_im), d_w_re.ptr, d_w_im.ptr, ptr(d_frf_re),
                                                          ptr(d_frf_im), ptr(d_fbb_re), ptr(d_fbb_im), ptr(d_eig), ptr(d_ustar_re),
                                                          ptr(d_ustar_im), ptr(d_rank)))

    def mu_jsdm_precoder(self, hests, ns, r_star, n_beams, groups=None, rank_tol=0.05, mode='pgp', unit_modulus=False, reg=None, cov=None,
                         keep_frf=False, keep_fbb=False, keep_eig=False):
        """The same from numpy arrays: hests = U complex arrays [npkt,nr,nt,234]; mode 'pgp' or 'jgp'; reg None, a scalar or [npkt]; cov None
        or complex [npkt, U, nt, nt] (a long-term covariance in place of the packet's own).  Returns (w_re, w_im float32 [npkt, U ns, nt,
        234]), then with keep_frf the analog part frf complex64 [npkt, nt, G n_beams], with keep_fbb the baseband part fbb complex64 [npkt,
        234, G n_beams, U ns], and with keep_eig the three of the first stage: eig float32 [npkt, G, nt], ustar complex64 [npkt, G, nt,
        r_star], rank int32 [npkt, G, 2] = (r_g, q_g)."""
        if mode not in ('pgp', 'jgp'):
            raise CsiError(-1, f"mu_jsdm_precoder: mode {mode!r} is not 'pgp' or 'jgp'")
        hests = [np.asarray(h) for h in hests]
        npkt = hests[0].shape[0] if hests and hests[0].ndim else 0
        for h in hests:
            if h.shape != (npkt, self.nr, self.nt, N_DATA):
                raise CsiError(-1, f'every h must be [{npkt},{self.nr},{self.nt},{N_DATA}], got {h.shape}')
        nu, m = len(hests), len(hests) * max(int(ns), 0)
        ng = nu if groups is None else (max([int(g) for g in groups] + [0]) + 1)
        q, rs = max(ng * int(n_beams), 0), max(int(r_star), 0)
        flags = (self.JSDM_PGP if mode == 'pgp' else 0) | (self.JSDM_UNIT_MODULUS if unit_modulus else 0)
        dev = [self.to_device(_f32c(h.real)) for h in hests] + [self.to_device(_f32c(h.imag)) for h in hests]
        d_reg = None if reg is None else self.to_device(np.ascontiguousarray(np.broadcast_to(np.asarray(reg, np.float32), (npkt,))))
        d_cov = [None, None]
        if cov is not None:
            cov = np.asarray(cov)
            if cov.shape != (npkt, nu, self.nt, self.nt):
                raise CsiError(-1, f'cov must be [{npkt},{nu},{self.nt},{self.nt}], got {cov.shape}')
            d_cov = [self.to_device(_f32c(cov.real)), self.to_device(_f32c(cov.imag))]
        outs = [self.empty((npkt, m, self.nt, N_DATA)) for _ in range(2)]
        frf = [self.empty((npkt, self.nt, q)) for _ in range(2)] if keep_frf else [None, None]
        fbb = [self.empty((npkt, N_DATA, q, m)) for _ in range(2)] if keep_fbb else [None, None]
        first = [None] * 4
        if keep_eig:
            first = [self.empty((npkt, ng, self.nt))] + [self.empty((npkt, ng, self.nt, rs)) if rs else None for _ in range(2)] + [self.empty((npkt, ng, 2))]
        try:
            self.mu_jsdm_precoder_device(dev[:nu], dev[nu:], npkt, ns, r_star, n_beams, outs[0], outs[1], groups, rank_tol, flags, d_reg,
                                         d_cov[0], d_cov[1], frf[0], frf[1], fbb[0], fbb[1], first[0], first[1], first[2], first[3])
            self.synchronize()
            res = [outs[0].download(), outs[1].download()]
            if keep_frf:
                res.append((frf[0].download() + 1j * frf[1].download()).astype(np.complex64))
            if keep_fbb:
                res.append((fbb[0].download() + 1j * fbb[1].download()).astype(np.complex64))
            if keep_eig:
                ustar = (first[1].download() + 1j * first[2].download()) if rs else np.zeros((npkt, ng, self.nt, 0))
                res += [first[0].download(), ustar.astype(np.complex64), first[3].download().view(np.int32)]
            return tuple(res)
        finally:
            for a in dev + outs + frf + fbb + first + d_cov + [d_reg]:
                if a is not None:
                    a.free()

    # ------------------------------------------------------------------ quantised CSI feedback (csrc/feedback.hip.h)
    FB_LAYOUT_W, FB_LAYOUT_CSI = 0, 1

    def feedback_compress_device(self, d_h_re, d_h_im, npkt, nc, b_phi, b_psi, ng=1, d_phi_code=None, d_psi_code=None, d_phi=None, d_psi=None,
                                 d_sigma=None, d_v_re=None, d_v_im=None):
        """Givens-angle report of the nc dominant right singular vectors of every (packet, reported carrier) of the planes d_h_re /
        d_h_im [npkt,nr,nt,234] (csi_feedback_compress_device): d_phi_code / d_psi_code hold uint16 [npkt, n_ang, n_rep] (arrays of
        (npkt n_ang n_rep + 1) // 2 floats serve), optional d_phi / d_psi float32 of the same shape, d_sigma [npkt, nc, n_rep], the pair
        d_v_re / d_v_im [npkt, nc, nt, n_rep]; n_ang = feedback.n_angles(nt, nc), n_rep = feedback.n_reports(ng).  b_phi = b_psi = 0: the
        continuous angles only.  Asynchronous, on the engine's stream."""
        ptr = lambda a: None if a is None else a.ptr
        self._check(self._lib.csi_feedback_compress_device(self._ctx, d_h_re.ptr, d_h_im.ptr, int(npkt), int(nc), int(b_phi), int(b_psi), int(ng),
                                                           ptr(d_phi_code), ptr(d_psi_code), ptr(d_phi), ptr(d_psi), ptr(d_sigma), ptr(d_v_re),
                                                           ptr(d_v_im)))

    def feedback_expand_device(self, npkt, nc, b_phi, b_psi, ng, layout, d_out_re, d_out_im, d_phi_code=None, d_psi_code=None, d_phi=None,
                               d_psi=None, d_sigma=None):
        """A report expanded at the base station (csi_feedback_expand_device) from the codes or from the continuous angles (exactly one
        pair): layout FB_LAYOUT_W - d_out_re / d_out_im [npkt, nc, nt, 234], sqrt(nt / nc) Vhat, what mu_link_sim_device reads with one
        user and ns = nc; FB_LAYOUT_CSI - [npkt, nr, nt, 234], row s < nc = sigma_s conj(Vhat[:, s]) (d_sigma None: 1), the other rows
        zero.  Asynchronous, on the engine's stream."""
        ptr = lambda a: None if a is None else a.ptr
        self._check(self._lib.csi_feedback_expand_device(self._ctx, ptr(d_phi_code), ptr(d_psi_code), ptr(d_phi), ptr(d_psi), ptr(d_sigma),
                                                         int(npkt), int(nc), int(b_phi), int(b_psi), int(ng), int(layout), d_out_re.ptr, d_out_im.ptr))

    def _u16_download(self, d, shape):
        n = int(np.prod(shape, dtype=np.int64))
        return d.download().view(np.uint16)[:n].reshape(shape).copy()

    def feedback_compress(self, h, nc, b_phi=0, b_psi=0, ng=1, keep_angles=False, keep_v=False):
        """The same from a complex array h [npkt,nr,nt,234] -> FeedbackReport: phi_code / psi_code uint16 [npkt, n_ang, n_rep] (None with
        b_phi = b_psi = 0), phi / psi float32 (with keep_angles, and always without bits), sigma float32 [npkt, nc, n_rep], v complex64
        [npkt, nc, nt, n_rep] with keep_v (the vectors that were decomposed)."""
        from . import feedback as fb
        h = np.asarray(h)
        if h.ndim != 4 or h.shape[1:] != (self.nr, self.nt, N_DATA):
            raise CsiError(-1, f'h must be [npkt,{self.nr},{self.nt},{N_DATA}], got {h.shape}')
        npkt, coded = h.shape[0], (int(b_phi), int(b_psi)) != (0, 0)
        ang = (npkt, max(fb.n_angles(self.nt, nc), 0), fb.n_reports(ng if ng in (1, 2, 4) else 1))
        words = ((int(np.prod(ang, dtype=np.int64)) + 1) // 2,)
        dev = [self.to_device(_f32c(h.real)), self.to_device(_f32c(h.imag))]
        codes = [self.empty(words) for _ in range(2)] if coded else [None, None]
        angles = [self.empty(ang) for _ in range(2)] if keep_angles or not coded else [None, None]
        sigma = self.empty((npkt, max(int(nc), 0), ang[2]))
        v = [self.empty((npkt, max(int(nc), 0), self.nt, ang[2])) for _ in range(2)] if keep_v else [None, None]
        try:
            self.feedback_compress_device(dev[0], dev[1], npkt, nc, b_phi, b_psi, ng, codes[0], codes[1], angles[0], angles[1], sigma, v[0], v[1])
            self.synchronize()
            return FeedbackReport(*[self._u16_download(c, ang) if c is not None else None for c in codes],
                                  *[a.download() if a is not None else None for a in angles], sigma.download(),
                                  (v[0].download() + 1j * v[1].download()).astype(np.complex64) if keep_v else None,
                                  int(nc), int(b_phi), int(b_psi), int(ng))
        finally:
            for a in dev + codes + angles + [sigma] + v:
                if a is not None:
                    a.free()

    def feedback_expand(self, report, layout='w', use_sigma=True, continuous=False):
        """A FeedbackReport expanded into complex64 planes: layout 'w' [npkt, nc, nt, 234] or 'csi' [npkt, nr, nt, 234] (use_sigma False:
        unit singular values).  The codes are used where the report has them, unless `continuous` asks for its angles."""
        if layout not in ('w', 'csi'):
            raise CsiError(-1, f"feedback_expand: layout {layout!r} is not 'w' or 'csi'")
        coded = report.phi_code is not None and not continuous
        src = (report.phi_code, report.psi_code) if coded else (report.phi, report.psi)
        if src[0] is None or src[1] is None:
            raise CsiError(-1, 'feedback_expand: the report holds neither codes nor angles to expand')
        npkt = src[0].shape[0]
        if coded:
            pad = [np.concatenate([np.ascontiguousarray(c, np.uint16).reshape(-1), np.zeros(c.size & 1, np.uint16)]).view(np.float32) for c in src]
            dev = [self.to_device(x) for x in pad]
        else:
            dev = [self.to_device(_f32c(x)) for x in src]
        d_sigma = self.to_device(_f32c(report.sigma)) if (use_sigma and layout == 'csi' and report.sigma is not None) else None
        outs = [self.empty((npkt, report.nc if layout == 'w' else self.nr, self.nt, N_DATA)) for _ in range(2)]
        try:
            kw = dict(d_phi_code=dev[0], d_psi_code=dev[1]) if coded else dict(d_phi=dev[0], d_psi=dev[1])
            self.feedback_expand_device(npkt, report.nc, report.b_phi, report.b_psi, report.ng, self.FB_LAYOUT_W if layout == 'w' else self.FB_LAYOUT_CSI,
                                        outs[0], outs[1], d_sigma=d_sigma, **kw)
            self.synchronize()
            return (outs[0].download() + 1j * outs[1].download()).astype(np.complex64)
        finally:
            for a in dev + outs + [d_sigma]:
                if a is not None:
                    a.free()

    # ------------------------------------------------------------------ receive combining (csrc/rx_combine.hip.h)
    def rx_combiner_device(self, d_hest_re, d_hest_im, npkt, ns, d_c_re, d_c_im, d_sigma=None):
        """The U^H combiner of the planes d_hest_re / d_hest_im [npkt,nr,nt,234] (csi_rx_combiner_device): d_c_re / d_c_im [npkt, ns, nr,
        234], row s = exp(i t_s) u_s^H of the s-th largest singular value, (C H)[s][nt-1] real and >= 0; optional d_sigma [npkt, ns, 234].
        Asynchronous, on the engine's stream."""
        self._check(self._lib.csi_rx_combiner_device(self._ctx, d_hest_re.ptr, d_hest_im.ptr, int(npkt), int(ns), d_c_re.ptr, d_c_im.ptr,
                                                     None if d_sigma is None else d_sigma.ptr))

    def rx_apply_combiner_device(self, d_c_re, d_c_im, d_h_re, d_h_im, npkt, ns, d_e_re, d_e_im):
        """E = C H of the combiner d_c_re / d_c_im [npkt, ns, nr, 234] and the planes d_h_re / d_h_im [npkt,nr,nt,234] into d_e_re / d_e_im
        [npkt,nr,nt,234] (csi_rx_apply_combiner_device): rows s < ns the combined streams, the other rows zero - what mu_link_sim_device
        takes as the channel of a combining user, and every estimate consumer as its report.  Asynchronous, on the engine's stream."""
        self._check(self._lib.csi_rx_apply_combiner_device(self._ctx, d_c_re.ptr, d_c_im.ptr, d_h_re.ptr, d_h_im.ptr, int(npkt), int(ns),
                                                           d_e_re.ptr, d_e_im.ptr))

    def rx_combiner(self, h, ns, keep_sigma=False):
        """The same from a complex array h [npkt,nr,nt,234] -> C complex64 [npkt, ns, nr, 234]; with keep_sigma (C, sigma float32 [npkt,
        ns, 234])."""
        h = np.asarray(h)
        if h.ndim != 4 or h.shape[1:] != (self.nr, self.nt, N_DATA):
            raise CsiError(-1, f'h must be [npkt,{self.nr},{self.nt},{N_DATA}], got {h.shape}')
        npkt, rows = h.shape[0], max(int(ns), 0)
        dev = [self.to_device(_f32c(h.real)), self.to_device(_f32c(h.imag))]
        outs = [self.empty((npkt, rows, self.nr, N_DATA)) for _ in range(2)]
        sigma = self.empty((npkt, rows, N_DATA)) if keep_sigma else None
        try:
            self.rx_combiner_device(dev[0], dev[1], npkt, ns, outs[0], outs[1], sigma)
            self.synchronize()
            c = (outs[0].download() + 1j * outs[1].download()).astype(np.complex64)
            return (c, sigma.download()) if keep_sigma else c
        finally:
            for a in dev + outs + [sigma]:
                if a is not None:
                    a.free()

    def rx_apply_combiner(self, C, h):
        """E = C H from complex arrays C [npkt, ns, nr, 234] and h [npkt,nr,nt,234] -> complex64 [npkt,nr,nt,234]."""
        C, h = np.asarray(C), np.asarray(h)
        if h.ndim != 4 or h.shape[1:] != (self.nr, self.nt, N_DATA):
            raise CsiError(-1, f'h must be [npkt,{self.nr},{self.nt},{N_DATA}], got {h.shape}')
        npkt = h.shape[0]
        if C.ndim != 4 or C.shape[0] != npkt or C.shape[2:] != (self.nr, N_DATA):
            raise CsiError(-1, f'C must be [{npkt},ns,{self.nr},{N_DATA}], got {C.shape}')
        dev = [self.to_device(_f32c(x)) for x in (C.real, C.imag, h.real, h.imag)]
        outs = [self.empty((npkt, self.nr, self.nt, N_DATA)) for _ in range(2)]
        try:
            self.rx_apply_combiner_device(dev[0], dev[1], dev[2], dev[3], npkt, C.shape[1], outs[0], outs[1])
            self.synchronize()
            return (outs[0].download() + 1j * outs[1].download()).astype(np.complex64)
        finally:
            for a in dev + outs:
                a.free()

    def viterbi_decode(self, llr):
        """Viterbi decoding of terminated codewords of the rate-1/3 K = 7 code (133, 171, 165): llr float [ncw, 3 n_steps], positive = 0
        -> uint8 [ncw, n_steps - 6] (csi_viterbi_decode_device; fp32 metrics, ties to the predecessor with the lower state number)."""
        llr = _f32c(llr)
        if llr.ndim != 2 or llr.shape[1] % 3:
            raise CsiError(-1, f'llr must be [ncw, 3 n_steps], got {llr.shape}')
        ncw, n_steps = llr.shape[0], llr.shape[1] // 3
        n_info = max(n_steps - 6, 0)
        d_llr, d_bits = self.to_device(llr), self.empty(((ncw * n_info + 3) // 4,))
        try:
            self._check(self._lib.csi_viterbi_decode_device(self._ctx, d_llr.ptr or None, ncw, n_steps, d_bits.ptr or None))
            self.synchronize()
            return d_bits.download().view(np.uint8)[:ncw * n_info].reshape(ncw, n_info).copy()
        finally:
            d_llr.free()
            d_bits.free()

    def capture_begin(self):
        """Record the device-pointer calls that follow (estimate_device, hybrid_weights_device, ...) into one hipGraph instead of
        running them.  Run the same calls once eagerly first, so that every buffer has its size.  Always close with capture_end."""
        self._check(self._lib.csi_capture_begin(self._ctx))

    def capture_end(self):
        """Close the capture; returns a CapturedGraph whose launch() replays the recorded calls on the engine's stream."""
        g = ctypes.c_void_p()
        self._check(self._lib.csi_capture_end(self._ctx, ctypes.byref(g)))
        return CapturedGraph(self, g.value)

    def predict_samples(self, model, x):
        """Literal Model.predict of one component: x [B, len_ltf+nt] -> float32 [B, n_out]."""
        idx = {'real': 0, 'imag': 1}.get(model, model)
        x = _f32c(x)
        if x.ndim != 2 or x.shape[1] != self.d_in:
            raise CsiError(-1, f'x must be [B,{self.d_in}], got {x.shape}')
        y = np.empty((x.shape[0], self.n_out), dtype=np.float32)
        self._check(self._lib.csi_predict_samples(self._ctx, int(idx), _fp(x), x.shape[0], _fp(y)))
        return y

    # ------------------------------------------------------------------ multi-GPU: RCCL inside the library
    def comm_init(self, rank, world, unique_id):
        """ncclCommInitRank on this engine's GPU (collective over the ranks); ``unique_id`` = the 128 bytes
        ``get_unique_id()`` produced on one rank (see ``dist.exchange_unique_id``)."""
        uid = bytes(unique_id)
        if len(uid) != 128:
            raise CsiError(-1, 'unique id must be 128 bytes')
        self._check(self._lib.csi_comm_init(self._ctx, int(rank), int(world), uid))

    def broadcast_weights(self, root=0):
        """Both component models and the pilot matrix as they sit on ``root``'s GPU -> every rank's GPU (ncclBroadcast of the
        device buffers, no host copy); afterwards every engine is loaded.  Returns the bytes moved."""
        self._check(self._lib.csi_broadcast_weights(self._ctx, int(root)))
        return self.get_option('comm_bytes')

    def clone_weights_from(self, other):
        """Both component models and the pilot matrix as they sit on ``other``'s GPU memory -> this engine (device to device, same
        process; the receiver side of ``broadcast_weights`` without RCCL).  The engines must agree in nt, hidden widths, n_out,
        use_bn and dtype; a mismatch raises and leaves this engine empty."""
        self._check(self._lib.csi_clone_weights(self._ctx, other._ctx))

    def comm_destroy(self):
        self._check(self._lib.csi_comm_destroy(self._ctx))

    # ------------------------------------------------------------------ device-resident calls
    def _checked(self, launch):
        """Run ``launch()`` (device-pointer calls), synchronise, and - if the split-f16 engine's range guard reports
        (CsiError code -6: an operand left the f16 range after scaling, or a whole row sat in its denormals) - run it
        again on the fp32 MFMA kernels, as the host-buffer entry points do by themselves.  Returns 'split', or 'fp32' when
        the repeat served the call; the option is put back either way (changing it drops cached hipGraphs)."""
        launch()
        try:
            self.synchronize()
            return 'split'
        except CsiError as err:
            if err.code != -6:
                raise
        engine = self.get_option('f32_engine')
        self.set_option('f32_engine', 0)
        try:
            launch()
            self.synchronize()
        finally:
            self.set_option('f32_engine', engine)
        self.range_recoveries = getattr(self, 'range_recoveries', 0) + 1
        return 'fp32'

    def predict_device(self, d_re, d_im, npkt, d_out_re, d_out_im, checked=False):
        """Asynchronous.  On the split-f16 engine a range-guard hit is reported by the NEXT ``synchronize()`` (CsiError
        code -6): outputs must not be consumed before it returned cleanly (the host-buffer calls repeat by themselves).
        ``checked=True`` does that for the caller: synchronises, repeats the call on the fp32 MFMA kernels if the guard
        reported, and returns which engine served it ('split' / 'fp32')."""
        def launch():
            self._check(self._lib.csi_predict_device(self._ctx, d_re.ptr, d_im.ptr, int(npkt), d_out_re.ptr, d_out_im.ptr))
        if checked:
            return self._checked(launch)
        launch()

    def estimate_device(self, d_re, d_im, npkt, d_out_re, d_out_im, d_h_re, d_h_im, checked=False):
        """LS + DNN of device-resident packets as one call (one hipGraph under 'use_graph'); ``checked`` as in predict_device."""
        def launch():
            self._check(self._lib.csi_estimate_device(self._ctx, d_re.ptr, d_im.ptr, int(npkt), d_out_re.ptr, d_out_im.ptr, d_h_re.ptr, d_h_im.ptr))
        if checked:
            return self._checked(launch)
        launch()

    def ls_estimate_device(self, d_re, d_im, npkt, d_h_re, d_h_im):
        self._check(self._lib.csi_ls_estimate_device(self._ctx, d_re.ptr, d_im.ptr, int(npkt), d_h_re.ptr, d_h_im.ptr))

    def nmse(self, h_ref, h_est):
        """NMSE_subk of the reference's evaluation (BER_test_maMIMO_LTF.m:675-686): per link
        ||ref - est||^2 / ||ref||^2 over the last axis, mean over all links.  Complex arrays of equal
        shape [..., n_bins] (e.g. the true channel and ``out_real + 1j * out_imag``)."""
        h_ref, h_est = np.asarray(h_ref), np.asarray(h_est)
        if h_ref.shape != h_est.shape or h_ref.ndim < 1 or h_ref.size == 0:
            raise CsiError(-1, f'h_ref and h_est must have the same non-empty shape, got {h_ref.shape} and {h_est.shape}')
        n_bins = h_ref.shape[-1]
        planes = [_f32c(a).reshape(-1, n_bins) for a in (h_ref.real, h_ref.imag, h_est.real, h_est.imag)]
        out = ctypes.c_double(0.0)
        self._check(self._lib.csi_nmse(self._ctx, _fp(planes[0]), _fp(planes[1]), _fp(planes[2]), _fp(planes[3]),
                                       planes[0].shape[0], n_bins, ctypes.byref(out)))
        return float(out.value)

    def nmse_device(self, d_ref_re, d_ref_im, d_est_re, d_est_im, nlinks, n_bins=N_DATA, d_per_link=None):
        """The same metric on device-resident planes ([nlinks][n_bins] float32 each); synchronous.
        ``d_per_link`` (a DeviceArray of nlinks floats) also receives the per-link ratios."""
        out = ctypes.c_double(0.0)
        self._check(self._lib.csi_nmse_device(self._ctx, d_ref_re.ptr, d_ref_im.ptr, d_est_re.ptr, d_est_im.ptr, int(nlinks), int(n_bins),
                                              d_per_link.ptr if d_per_link is not None else None, ctypes.byref(out)))
        return float(out.value)

    def synth_white(self, seed, first_pkt, npkt, d_re, d_im):
        self._check(self._lib.csi_synth_white(self._ctx, int(seed), int(first_pkt), int(npkt), d_re.ptr, d_im.ptr))

    def synth_structured(self, seed, first_pkt, npkt, snr_db=None, n_taps=8, amp_scale=True, want_channel=True, want_noise_std=True):
        """Known-channel sounding packets generated on the device (csi_synth_structured): packets first_pkt .. first_pkt + npkt - 1
        of the stream `seed`.  snr_db: None (noise-free), a scalar or one level per packet, relative to each packet's own power.
        Returns DeviceArrays (ltf_re, ltf_im [npkt][nr][len_ltf], h_re, h_im [npkt][nr][nt][234], noise_std [npkt]); the channel
        planes / noise_std are None when not wanted.  h is what ls_estimate_device returns for the noise-free packet when
        P P^T = Nt I; noise_std is the deviation per real component before the amplitude scale.  Asynchronous."""
        npkt = int(npkt)
        if npkt < 0:
            raise CsiError(-1, f'csi_synth_structured: npkt {npkt} must not be negative')
        snr = None
        if snr_db is not None:
            snr = np.ascontiguousarray(np.broadcast_to(np.asarray(snr_db, dtype=np.float32), (npkt,)))
        d_re, d_im = self.empty((npkt, self.nr, SYM_LEN * self.nt)), self.empty((npkt, self.nr, SYM_LEN * self.nt))
        d_h = [self.empty((npkt, self.nr, self.nt, N_DATA)) for _ in range(2)] if want_channel else [None, None]
        d_std = self.empty((npkt,)) if want_noise_std else None
        self._check(self._lib.csi_synth_structured(self._ctx, int(seed), int(first_pkt), npkt, _fp(snr) if snr is not None else None,
                                                   int(n_taps), 1 if amp_scale else 0, d_re.ptr or None, d_im.ptr or None,
                                                   d_h[0].ptr if want_channel else None, d_h[1].ptr if want_channel else None,
                                                   d_std.ptr if want_noise_std else None))
        return d_re, d_im, d_h[0], d_h[1], d_std

    @staticmethod
    def _scatter_config(who, npkt, n_scat, range_m, az_deg, el_deg, box_frac, random_users, amp_scale, sample_rate_hz):
        """The csi_scatter_config of the scattering entry points from their keyword arguments; `who` names the entry point in a refusal"""
        if npkt < 0:
            raise CsiError(-1, f'{who}: npkt {npkt} must not be negative')
        if n_scat < 1 or n_scat > 256:
            raise CsiError(-1, f'{who}: n_scat {n_scat} outside 1 .. 256')
        for name, val in (('range_m', range_m), ('box_frac', box_frac), ('sample_rate_hz', sample_rate_hz)):
            if not (np.isfinite(val) and val > 0):      # a zero would select the default of the C configuration
                raise CsiError(-1, f'{who}: {name} {val} must be finite and positive')
        az = float(az_deg)
        return _lib.CsiScatterConfig(n_scat=n_scat, flags=(1 if amp_scale else 0) | (2 if random_users else 0), range_m=float(range_m),
                                     az_deg=360.0 if az == 0.0 else az, el_deg=float(el_deg), box_frac=float(box_frac),
                                     sample_rate_hz=float(sample_rate_hz))

    def synth_scattering(self, seed, first_pkt, npkt, snr_db=None, n_scat=100, range_m=100.0, az_deg=30.0, el_deg=0.0, box_frac=0.1,
                         random_users=False, amp_scale=True, want_channel=True, want_noise_std=True, want_tau=False,
                         sample_rate_hz=100e6):
        """Known-channel sounding packets of the geometric single-bounce scattering channel (csi_synth_scattering):
        n_scat scatterers in a box of half edge box_frac * range around a user at (range_m, az_deg, el_deg) - or at a position
        drawn per packet (random_users) - seen from half-wavelength ULAs.  Everything else as synth_structured, whose tuple it
        returns plus tau: a DeviceArray [npkt][n_scat] of the absolute path delays in samples (None unless want_tau), the hvec
        rows the reference hands its LMMSE smoother.  Asynchronous."""
        npkt, n_scat = int(npkt), int(n_scat)
        cfg = self._scatter_config('csi_synth_scattering', npkt, n_scat, range_m, az_deg, el_deg, box_frac, random_users, amp_scale, sample_rate_hz)
        snr = None
        if snr_db is not None:
            snr = np.ascontiguousarray(np.broadcast_to(np.asarray(snr_db, dtype=np.float32), (npkt,)))
        d_re, d_im = self.empty((npkt, self.nr, SYM_LEN * self.nt)), self.empty((npkt, self.nr, SYM_LEN * self.nt))
        d_h = [self.empty((npkt, self.nr, self.nt, N_DATA)) for _ in range(2)] if want_channel else [None, None]
        d_std = self.empty((npkt,)) if want_noise_std else None
        d_tau = self.empty((npkt, n_scat)) if want_tau else None
        self._check(self._lib.csi_synth_scattering(self._ctx, int(seed), int(first_pkt), npkt, _fp(snr) if snr is not None else None,
                                                   ctypes.byref(cfg), d_re.ptr or None, d_im.ptr or None,
                                                   d_h[0].ptr if want_channel else None, d_h[1].ptr if want_channel else None,
                                                   d_std.ptr if want_noise_std else None, d_tau.ptr if want_tau else None))
        return d_re, d_im, d_h[0], d_h[1], d_std, d_tau

    def scatter_channel_at_device(self, seed, first_pkt, npkt, times_s, d_h_re, d_h_im, speed_mps=0.0, heading_az_deg=0.0, heading_el_deg=0.0,
                                  carrier_hz=28e9, random_heading=False, amp_scale=True, n_scat=100, range_m=100.0, az_deg=30.0, el_deg=0.0,
                                  box_frac=0.1, random_users=False, sample_rate_hz=100e6):
        """Channel aging (csi_scatter_channel_at_device): the true channel of synth_scattering's packets first_pkt ..
        first_pkt + npkt - 1 of stream `seed` at the times times_s (seconds, 1 .. 16 of them, any sign and order) for a user that
        moves with speed_mps along (heading_az_deg, heading_el_deg) in the transmitter's frame - or along an azimuth drawn per packet
        (random_heading).  d_h_re / d_h_im [n_times][npkt][nr][nt][234]: slice t is a plane pair like synth_scattering's h, and IS
        that h, bit for bit, at t = 0 or speed 0.  The scattering keywords are synth_scattering's.  One launch, asynchronous."""
        npkt, n_scat = int(npkt), int(n_scat)
        who = 'csi_scatter_channel_at_device'
        cfg = self._scatter_config(who, npkt, n_scat, range_m, az_deg, el_deg, box_frac, random_users, amp_scale, sample_rate_hz)
        if not (np.isfinite(carrier_hz) and carrier_hz > 0):      # a zero would select the default of the C record
            raise CsiError(-1, f'{who}: carrier_hz {carrier_hz} must be finite and positive')
        t = np.ascontiguousarray(np.atleast_1d(np.asarray(times_s, dtype=np.float64)))
        if t.ndim != 1:
            raise CsiError(-1, f'{who}: times_s must be a scalar or a vector, got shape {t.shape}')
        motion = _lib.CsiMotionConfig(speed_mps=float(speed_mps), heading_az_deg=float(heading_az_deg), heading_el_deg=float(heading_el_deg),
                                      carrier_hz=float(carrier_hz), flags=1 if random_heading else 0)
        self._check(self._lib.csi_scatter_channel_at_device(self._ctx, int(seed), int(first_pkt), npkt, ctypes.byref(cfg), ctypes.byref(motion),
                                                            t.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(t.size),
                                                            d_h_re.ptr or None, d_h_im.ptr or None))

    def scatter_channel_at(self, seed, first_pkt, npkt, times_s, **kw):
        """scatter_channel_at_device into two new DeviceArrays [n_times, npkt, nr, nt, 234], which it returns (h_re, h_im)"""
        n_times = int(np.atleast_1d(np.asarray(times_s)).size)
        d_h = [self.empty((n_times, int(npkt), self.nr, self.nt, N_DATA)) for _ in range(2)]
        self.scatter_channel_at_device(seed, first_pkt, npkt, times_s, d_h[0], d_h[1], **kw)
        return d_h[0], d_h[1]

    # ------------------------------------------------------------------ channel forecast (csrc/forecast.hip.h)
    def forecast_gram_device(self, d_x_re, d_x_im, npkt, d_t_re, d_t_im):
        """Gram matrix of P = len(d_x_re) soundings per (packet, rx) (csi_forecast_gram_device): d_x_re / d_x_im lists of DeviceArrays
        [npkt,nr,nt,234], oldest first; T[i][q] = sum conj(x_i) x_q into d_t_re / d_t_im [npkt,nr,P,P].  Asynchronous."""
        self._check(self._lib.csi_forecast_gram_device(self._ctx, self._ptr_array(d_x_re), self._ptr_array(d_x_im), len(d_x_re), int(npkt),
                                                       d_t_re.ptr or None, d_t_im.ptr or None))

    def forecast_gram_blocks_device(self, d_x_re, d_x_im, n_blocks, block_floats, d_t_re, d_t_im):
        """The same kernel on n_blocks blocks of block_floats contiguous floats per plane (csi_forecast_gram_blocks_device): T
        [n_blocks,P,P].  forecast_gram_device is the case (npkt nr, 234 nt)."""
        self._check(self._lib.csi_forecast_gram_blocks_device(self._ctx, self._ptr_array(d_x_re), self._ptr_array(d_x_im), len(d_x_re), int(n_blocks),
                                                              int(block_floats), d_t_re.ptr or None, d_t_im.ptr or None))

    def forecast_fit_device(self, d_t_re, d_t_im, n_snd, npkt, order, steps, d_c_re, d_c_im, ridge=1e-5, pool_rx=False, d_fit_err=None, d_info=None):
        """The predictor of every (packet, rx) from its Gram matrix (csi_forecast_fit_device): normal equations of order `order` for a
        horizon of `steps` sounding intervals, ridge * trace / order on the diagonal, fp64 Cholesky; c into d_c_re / d_c_im
        [npkt,nr,order].  pool_rx: one fit per packet from the summed systems of its rx antennas.  d_fit_err float [npkt,nr], d_info
        [npkt,nr] int32 bits in a DeviceArray (1 = the fallback c = (1, 0, ..) was taken), both optional.  Asynchronous."""
        self._check(self._lib.csi_forecast_fit_device(self._ctx, d_t_re.ptr or None, d_t_im.ptr or None, int(n_snd), int(npkt), int(order), int(steps),
                                                      float(ridge), 1 if pool_rx else 0, d_c_re.ptr or None, d_c_im.ptr or None,
                                                      d_fit_err.ptr if d_fit_err is not None else None, d_info.ptr if d_info is not None else None))

    def forecast_apply_device(self, d_x_re, d_x_im, npkt, order, d_c_re, d_c_im, d_out_re, d_out_im):
        """y = sum_m c_m x_{P-1-m} per (packet, rx) (csi_forecast_apply_device).  Asynchronous."""
        self._check(self._lib.csi_forecast_apply_device(self._ctx, self._ptr_array(d_x_re), self._ptr_array(d_x_im), len(d_x_re), int(npkt), int(order),
                                                        d_c_re.ptr or None, d_c_im.ptr or None, d_out_re.ptr or None, d_out_im.ptr or None))

    def forecast_device(self, d_x_re, d_x_im, npkt, order, steps, d_out_re, d_out_im, ridge=1e-5, pool_rx=False, d_c_re=None, d_c_im=None,
                        d_fit_err=None, d_info=None):
        """Gram, fit and apply in sequence (csi_forecast_device), the same bits as the three calls; T and, without d_c_re / d_c_im, c
        live in the engine's workspace (inside a capture an eager call of the same shape must have sized it).  Asynchronous."""
        opt = [a.ptr if a is not None else None for a in (d_c_re, d_c_im, d_fit_err, d_info)]
        self._check(self._lib.csi_forecast_device(self._ctx, self._ptr_array(d_x_re), self._ptr_array(d_x_im), len(d_x_re), int(npkt), int(order), int(steps),
                                                  float(ridge), 1 if pool_rx else 0, d_out_re.ptr or None, d_out_im.ptr or None, *opt))

    def sounding_noise_device(self, seed, first_pkt, npkt, d_err_var, d_x_re, d_x_im, d_out_re=None, d_out_im=None):
        """White estimation error on a CSI plane pair (csi_sounding_noise_device): out = x + sqrt(v / 2) (n_re + i n_im) with v =
        d_err_var [npkt,nr] and the normals of the noise stream of packets first_pkt .. of `seed`; in place without out planes.
        Asynchronous."""
        d_out_re = d_x_re if d_out_re is None else d_out_re
        d_out_im = d_x_im if d_out_im is None else d_out_im
        self._check(self._lib.csi_sounding_noise_device(self._ctx, int(seed), int(first_pkt), int(npkt), d_err_var.ptr or None, d_x_re.ptr or None,
                                                        d_x_im.ptr or None, d_out_re.ptr or None, d_out_im.ptr or None))

    def forecast(self, x, order, steps, ridge=1e-5, pool_rx=False, details=False):
        """Channel forecast from host arrays (csi_forecast): x complex [P,npkt,nr,nt,234], the soundings oldest first and equally
        spaced; returns the forecast of the channel `steps` intervals behind the newest one, complex64 [npkt,nr,nt,234].  With
        ``details`` also (c complex64 [npkt,nr,order], fit_err float32 [npkt,nr], info int32 [npkt,nr])."""
        x = np.asarray(x)
        if x.ndim != 5 or x.shape[2:] != (self.nr, self.nt, N_DATA):
            raise CsiError(-1, f'x must be [P,npkt,{self.nr},{self.nt},{N_DATA}], got {x.shape}')
        P, npkt = x.shape[:2]
        re, im = [_f32c(x[i].real) for i in range(P)], [_f32c(x[i].imag) for i in range(P)]
        host = lambda planes: (ctypes.c_void_p * max(P, 1))(*[a.ctypes.data for a in planes])      # noqa: E731
        o_re, o_im = np.empty((npkt, self.nr, self.nt, N_DATA), np.float32), np.empty((npkt, self.nr, self.nt, N_DATA), np.float32)
        m = max(int(order), 0)
        c_re, c_im = np.empty((npkt, self.nr, m), np.float32), np.empty((npkt, self.nr, m), np.float32)
        fit_err, info = np.empty((npkt, self.nr), np.float32), np.empty((npkt, self.nr), np.int32)
        self._check(self._lib.csi_forecast(self._ctx, host(re), host(im), P, npkt, int(order), int(steps), float(ridge), 1 if pool_rx else 0,
                                           _fp(o_re), _fp(o_im), _fp(c_re), _fp(c_im), _fp(fit_err), info.ctypes.data))
        out = self._c64(o_re, o_im)
        return (out, self._c64(c_re, c_im), fit_err, info) if details else out

    # ------------------------------------------------------------------ carrier frequency offset (csrc/cfo.hip.h)
    def cfo_estimate_device(self, d_ltf_re, d_ltf_im, npkt, d_eps, cp_skip=0, d_quality=None):
        """The carrier frequency offset of every packet from the cyclic prefixes of its sounding symbols (csi_cfo_estimate_device):
        d_eps [npkt] as float64 in subcarrier spacings (an array of 2 float32 words per packet, as null_noise_device's), optional
        d_quality [npkt] = |gamma| / E, about snr / (1 + snr); cp_skip 0 .. 63 leaves out the head of every prefix.  Asynchronous."""
        self._check(self._lib.csi_cfo_estimate_device(self._ctx, d_ltf_re.ptr or None, d_ltf_im.ptr or None, int(npkt), int(cp_skip), d_eps.ptr or None,
                                                      d_quality.ptr if d_quality is not None else None))

    def cfo_rotate_device(self, d_in_re, d_in_im, npkt, d_eps, scale, d_out_re=None, d_out_im=None):
        """y[p,r,n] = x[p,r,n] exp(2 pi i scale eps[p] n / 256) on device-resident preambles (csi_cfo_rotate_device): d_eps [npkt] as
        float64 (2 float32 words per packet); scale +1 impairs, -1 corrects; in place without out planes.  Asynchronous."""
        d_out_re = d_in_re if d_out_re is None else d_out_re
        d_out_im = d_in_im if d_out_im is None else d_out_im
        self._check(self._lib.csi_cfo_rotate_device(self._ctx, d_in_re.ptr or None, d_in_im.ptr or None, int(npkt), d_eps.ptr or None, float(scale),
                                                    d_out_re.ptr or None, d_out_im.ptr or None))

    def cfo_correct_device(self, d_ltf_re, d_ltf_im, npkt, d_out_re=None, d_out_im=None, cp_skip=0, d_eps=None, d_quality=None):
        """Estimate, then rotate by -eps_hat (csi_cfo_correct_device): two launches, the bits of the two calls; in place without out
        planes; optional d_eps [npkt] as float64 and d_quality [npkt] receive the estimate.  Asynchronous."""
        d_out_re = d_ltf_re if d_out_re is None else d_out_re
        d_out_im = d_ltf_im if d_out_im is None else d_out_im
        self._check(self._lib.csi_cfo_correct_device(self._ctx, d_ltf_re.ptr or None, d_ltf_im.ptr or None, int(npkt), int(cp_skip), d_out_re.ptr or None,
                                                     d_out_im.ptr or None, d_eps.ptr if d_eps is not None else None,
                                                     d_quality.ptr if d_quality is not None else None))

    def cfo_correct(self, ltf, cp_skip=0, details=False):
        """Carrier-frequency-offset correction from host arrays (csi_cfo_correct): ltf complex [npkt,nr,len_ltf]; returns the corrected
        preambles, complex64 of the same shape.  With ``details`` also (eps_hat float64 [npkt], quality float32 [npkt])."""
        re, im = self._split(ltf, None)
        npkt = re.shape[0]
        o_re, o_im = np.empty_like(re), np.empty_like(im)
        eps, quality = np.empty(npkt, np.float64), np.empty(npkt, np.float32)
        self._check(self._lib.csi_cfo_correct(self._ctx, _fp(re), _fp(im), npkt, int(cp_skip), _fp(o_re), _fp(o_im), eps.ctypes.data, _fp(quality)))
        out = self._c64(o_re, o_im)
        return (out, eps, quality) if details else out

    # ------------------------------------------------------------------ symbol timing (csrc/sync.hip.h)
    def sync_embed_device(self, seed, first_pkt, npkt, span, d_theta, d_x_re, d_x_im, d_cap_re, d_cap_im, d_margin_std=None):
        """Packets [npkt][nr][len_ltf] placed at d_theta [npkt] (int32 words in a float32 DeviceArray; 0 .. span, clamped) inside capture
        planes [npkt][nr][len_ltf + span] (csi_sync_embed_device); the margins are noise of deviation d_margin_std [npkt] per real
        component from the stream (seed, first_pkt + p), zero without it.  Asynchronous."""
        self._check(self._lib.csi_sync_embed_device(self._ctx, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_pkt), int(npkt), int(span), d_theta.ptr or None,
                                                    d_margin_std.ptr if d_margin_std is not None else None, d_x_re.ptr or None, d_x_im.ptr or None,
                                                    d_cap_re.ptr or None, d_cap_im.ptr or None))

    def sync_estimate_device(self, d_cap_re, d_cap_im, npkt, span, d_theta, rho=1.0, d_eps=None, d_quality=None, d_metric=None):
        """Where every packet starts inside its capture, and its carrier frequency offset, from the cyclic prefixes
        (csi_sync_estimate_device): d_theta [npkt] int32 words = the lowest argmax of |gamma| - rho Phi over 0 .. span; optional d_eps
        [npkt] as float64 (2 float32 words per packet), d_quality [npkt], d_metric [npkt][span + 1] as float64.  Asynchronous."""
        opt = lambda d: d.ptr if d is not None else None      # noqa: E731
        self._check(self._lib.csi_sync_estimate_device(self._ctx, d_cap_re.ptr or None, d_cap_im.ptr or None, int(npkt), int(span), float(rho),
                                                       d_theta.ptr or None, opt(d_eps), opt(d_quality), opt(d_metric)))

    def sync_extract_device(self, d_cap_re, d_cap_im, npkt, span, d_theta, d_out_re, d_out_im, d_eps=None):
        """y[p,r,n] = c[p,r,theta[p] + n] exp(-2 pi i eps[p] n / 256) (csi_sync_extract_device): the packet cut out of its capture at
        d_theta (clamped into 0 .. span), a copy of the bits without d_eps.  Asynchronous."""
        self._check(self._lib.csi_sync_extract_device(self._ctx, d_cap_re.ptr or None, d_cap_im.ptr or None, int(npkt), int(span), d_theta.ptr or None,
                                                      d_eps.ptr if d_eps is not None else None, d_out_re.ptr or None, d_out_im.ptr or None))

    def sync_correct_device(self, d_cap_re, d_cap_im, npkt, span, d_out_re, d_out_im, rho=1.0, remove_cfo=True, d_theta=None, d_eps=None, d_quality=None):
        """Estimate, then cut out at theta_hat, with ``remove_cfo`` also removing eps_hat (csi_sync_correct_device): two launches, the
        bits of the two calls; optional d_theta / d_eps / d_quality receive the estimate.  Asynchronous."""
        opt = lambda d: d.ptr if d is not None else None      # noqa: E731
        self._check(self._lib.csi_sync_correct_device(self._ctx, d_cap_re.ptr or None, d_cap_im.ptr or None, int(npkt), int(span), float(rho),
                                                      1 if remove_cfo else 0, d_out_re.ptr or None, d_out_im.ptr or None, opt(d_theta), opt(d_eps),
                                                      opt(d_quality)))

    def sync_correct(self, capture, span, rho=1.0, remove_cfo=True, details=False):
        """Timing (and carrier-frequency-offset) correction from host arrays (csi_sync_correct): capture complex
        [npkt,nr,len_ltf + span]; returns the packets cut out at theta_hat, complex64 [npkt,nr,len_ltf].  With ``details`` also
        (theta_hat int32 [npkt], eps_hat float64 [npkt], quality float32 [npkt])."""
        capture = np.asarray(capture)
        re, im = _f32c(capture.real), _f32c(capture.imag)
        if re.ndim != 3 or re.shape[1:] != (self.nr, self.len_ltf + int(span)):
            raise CsiError(-1, f'captures must be [npkt,{self.nr},{self.len_ltf + int(span)}], got {re.shape}')
        npkt = re.shape[0]
        o_re, o_im = (np.empty((npkt, self.nr, self.len_ltf), np.float32) for _ in range(2))
        theta, eps, quality = np.empty(npkt, np.int32), np.empty(npkt, np.float64), np.empty(npkt, np.float32)
        self._check(self._lib.csi_sync_correct(self._ctx, _fp(re), _fp(im), npkt, int(span), float(rho), 1 if remove_cfo else 0, _fp(o_re), _fp(o_im),
                                               theta.ctypes.data, eps.ctypes.data, _fp(quality)))
        out = self._c64(o_re, o_im)
        return (out, theta, eps, quality) if details else out

    def lmmse_estimate_device(self, d_h_re, d_h_im, npkt, d_hvec, L, d_snr_db, d_out_re, d_out_im):
        """LMMSE smoothing of device-resident LS planes (csi_lmmse_estimate_device): d_hvec [npkt][L], d_snr_db [npkt][nr]; asynchronous."""
        self._check(self._lib.csi_lmmse_estimate_device(self._ctx, d_h_re.ptr, d_h_im.ptr, int(npkt), d_hvec.ptr, int(L), d_snr_db.ptr,
                                                        d_out_re.ptr, d_out_im.ptr))

    def lmmse_blind_device(self, d_ltf_re, d_ltf_im, d_h_re, d_h_im, npkt, d_out_re, d_out_im, d_noise_var=None, d_corr=None):
        """LMMSE smoothing of device-resident LS planes from the packets' own statistics (csi_lmmse_blind_device): the preamble planes the
        LS estimate was made from, out planes like h (they may be the h planes themselves); optional d_noise_var [npkt][nr] and d_corr
        [npkt][nr][234][2] receive the statistics as float64 (arrays of 2 and 2 * 468 float32 words per (packet, rx)); asynchronous."""
        self._check(self._lib.csi_lmmse_blind_device(self._ctx, d_ltf_re.ptr, d_ltf_im.ptr, d_h_re.ptr, d_h_im.ptr, int(npkt), d_out_re.ptr,
                                                     d_out_im.ptr, d_noise_var.ptr if d_noise_var is not None else None,
                                                     d_corr.ptr if d_corr is not None else None))

    def subspace_smooth_device(self, d_h_re, d_h_im, npkt, d_out_re, d_out_im, d_w=None):
        """Subspace smoother on device-resident planes (csi_subspace_smooth_device): out planes like h (they may be the h planes
        themselves), d_w [npkt][nr][rank] or None for the plain projection; one launch, asynchronous."""
        self._check(self._lib.csi_subspace_smooth_device(self._ctx, d_h_re.ptr, d_h_im.ptr, int(npkt), d_w.ptr if d_w is not None else None,
                                                         d_out_re.ptr, d_out_im.ptr))

    def beam_power_device(self, d_h_re, d_h_im, npkt, d_power):
        """Beam power on device-resident planes (csi_beam_power_device): d_power [npkt][nr][nb]; one launch, asynchronous."""
        self._check(self._lib.csi_beam_power_device(self._ctx, d_h_re.ptr, d_h_im.ptr, int(npkt), d_power.ptr))

    def beam_smooth_device(self, d_h_re, d_h_im, npkt, d_out_re, d_out_im, d_w=None):
        """Beam-space smoother on device-resident planes (csi_beam_smooth_device): out planes like h (they may be the h planes
        themselves), d_w [npkt][nr][nb] or None for the plain projection; one launch, asynchronous."""
        self._check(self._lib.csi_beam_smooth_device(self._ctx, d_h_re.ptr, d_h_im.ptr, int(npkt), d_w.ptr if d_w is not None else None,
                                                     d_out_re.ptr, d_out_im.ptr))

    def beam_wiener_device(self, d_h_re, d_h_im, npkt, d_err_var, d_out_re, d_out_im, d_w=None):
        """Beam-space Wiener smoother on device-resident planes (csi_beam_wiener_device): d_err_var [npkt][nr], out planes like h (they
        may be the h planes themselves), optional d_w [npkt][nr][nb] receives the weights; three launches, asynchronous."""
        self._check(self._lib.csi_beam_wiener_device(self._ctx, d_h_re.ptr, d_h_im.ptr, int(npkt), d_err_var.ptr, d_out_re.ptr, d_out_im.ptr,
                                                     d_w.ptr if d_w is not None else None))

    def null_noise_device(self, d_ltf_re, d_ltf_im, npkt, d_noise_var):
        """The null-carrier noise level of device-resident preambles (csi_null_noise_device): d_noise_var [npkt][nr] as float64 (an
        array of 2 float32 words per (packet, rx)); asynchronous."""
        self._check(self._lib.csi_null_noise_device(self._ctx, d_ltf_re.ptr, d_ltf_im.ptr, int(npkt), d_noise_var.ptr))

    # ------------------------------------------------------------------ profiling
    def profile_enable(self, on=True):
        self._check(self._lib.csi_profile_enable(self._ctx, int(bool(on))))

    def profile_reset(self):
        self._check(self._lib.csi_profile_reset(self._ctx))

    def pcie_probe(self, h2d_bytes, d2h_bytes):
        """(ms up alone, ms down alone, ms both at once) for these byte counts between pinned host memory and the device on two
        copy streams: the floor of a host-buffer call that moves them (csi_profile_pcie)."""
        a, b, ab = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        self._check(self._lib.csi_profile_pcie(self._ctx, int(h2d_bytes), int(d2h_bytes), ctypes.byref(a), ctypes.byref(b), ctypes.byref(ab)))
        return a.value, b.value, ab.value

    def band_skeleton(self, rows, iters=5):
        """(ms per launch, executed f16 TFLOP/s) of the fused per-pair kernel's MFMA + barrier skeleton on the loaded model's own
        operand data: the practical ceiling of that kernel on this part (csi_profile_band_skeleton)."""
        ms, fl = ctypes.c_double(), ctypes.c_double()
        self._check(self._lib.csi_profile_band_skeleton(self._ctx, int(rows), int(iters), ctypes.byref(ms), ctypes.byref(fl)))
        return ms.value, fl.value / (ms.value * 1e-3) / 1e12

    def profile(self):
        """dict kernel-name -> {ms, launches, flops, bytes} since the last reset."""
        out = {}
        for k in range(self._lib.csi_profile_num_kernels()):
            ms, n = ctypes.c_double(), ctypes.c_int64()
            fl, by = ctypes.c_double(), ctypes.c_double()
            self._check(self._lib.csi_profile_query(self._ctx, k, ctypes.byref(ms), ctypes.byref(n),
                                                    ctypes.byref(fl), ctypes.byref(by)))
            out[self._lib.csi_profile_kernel_name(k).decode()] = dict(
                ms=ms.value, launches=n.value, flops=fl.value, bytes=by.value)
        return out
