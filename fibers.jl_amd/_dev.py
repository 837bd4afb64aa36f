"""The device tier's argument contract and launch context ("The device tier in Python").  The fibd_* entries take bare pointers and
cannot know how long a buffer is or where it lives: every `*_device` function checks each tensor here (`tensor`: inputs and a
caller's outputs alike), launches inside `Launch` and takes its scratch from `work`.  A bad argument is an `ArgError` before any
launch."""
import ctypes as C

from . import _lib


class ArgError(ValueError, TypeError):
    """a device-tier argument that would be an out-of-bounds access or a wrong-device launch"""


def float3(v):
    """the `const float[3]` argument of the C ABI (voxel sizes)"""
    return (C.c_float * 3)(*[float(x) for x in v])


def _index(ref):
    d = ref.device                                          # a tensor's torch.device, or a plan's device index
    return d if isinstance(d, int) else d.index


def tensor(t, dtype, what, ref=None, n=None, unit=None, shape=None, bool_ok=False):
    """The one check: `t` is a contiguous CUDA torch.Tensor of `dtype` (one, a tuple of them, or None = any) and, where given, on the
    device of `ref` (a tensor, or a plan: this is the plan check), of exactly `n` elements, of a whole multiple of `unit` elements (at
    least one unit), of `shape` (None = any extent; its length is the rank).  bool_ok: a bool tensor passes as uint8.  Returns the
    tensor (the uint8 view of a bool one)."""
    import torch
    ok = isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous()
    if ok and bool_ok and t.dtype == torch.bool:
        t = t.view(torch.uint8)
    if ok and dtype is not None:
        ok = t.dtype in (dtype if isinstance(dtype, tuple) else (dtype,))
    if ok and ref is not None:
        ok = t.device.index == _index(ref)
    if ok and n is not None:
        ok = t.numel() == n
    if ok and unit is not None:
        ok = unit > 0 and t.numel() >= unit and t.numel() % unit == 0
    if ok and shape is not None:
        ok = t.dim() == len(shape)
        for s, w in zip(t.shape, shape) if ok else ():        # (a plain loop: this runs on every tracer call)
            if w is not None and s != w:
                ok = False
    if not ok:
        want = ["" if dtype is None else " " + " or ".join(str(d) for d in (dtype if isinstance(dtype, tuple) else (dtype,)))]
        want.append(" CUDA tensor")
        if shape is not None:
            want.append(" [%s]" % ", ".join("n" if w is None else str(w) for w in shape))
        if n is not None:
            want.append(" of %d elements" % n)
        if unit is not None:
            want.append(" of a whole multiple (at least one) of %d elements" % unit)
        if ref is not None:
            want.append(" on device %s" % _index(ref))
        got = "%s %s on %s%s" % (tuple(t.shape), t.dtype, t.device, "" if t.is_contiguous() else ", not contiguous") \
            if isinstance(t, torch.Tensor) else type(t).__name__
        raise ArgError("%s must be a contiguous%s, not %s" % (what, "".join(want), got))
    return t


def fit_args(plan, dwi, mask):
    """the inputs of a plan's fit: dwi float32 [plan.nvol, nvox], mask uint8 [nvox], both on the plan's device -> nvox"""
    import torch
    nvox = tensor(mask, torch.uint8, "mask", ref=plan).numel()
    tensor(dwi, torch.float32, "dwi [nvol, nvox]", ref=plan, n=nvox * plan.nvol)
    return nvox


def points(xyz, what="xyz", ref=None):
    """float32 [npoints, 3] (on the device of `ref`) -> npoints"""
    import torch
    if tensor(xyz, torch.float32, what, ref=ref).numel() % 3:
        raise ArgError("%s must hold whole points [npoints, 3], not %d coordinates" % (what, xyz.numel()))
    return xyz.numel() // 3


def lines(xyz, npts):
    """the checks every tract tool starts with: xyz float32 [npoints, 3], npts int32 [nlines] on its device -> (npoints, nlines)"""
    import torch
    return points(xyz), tensor(npts, torch.int32, "npts", ref=xyz).numel()


def stream_ptr(stream):
    """None (the current stream), a torch stream or a raw hipStream_t handle (an integer or a ctypes.c_void_p) -> the handle the
    fibd_* entries take"""
    if stream is None:
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)
    h = getattr(stream, "cuda_stream", stream)
    return h if isinstance(h, C.c_void_p) else C.c_void_p(h)


def torch_stream(stream):
    """None, a torch.cuda.Stream or a raw hipStream_t handle -> the torch stream object (None: torch's current stream)"""
    import torch
    if stream is None or isinstance(stream, torch.cuda.Stream):
        return stream
    handle = int(getattr(stream, "value", stream) or 0)        # ctypes.c_void_p (the package's own handle type) or a plain integer
    if handle == 0:                                             # the null stream: torch's default stream
        return torch.cuda.default_stream()
    return torch.cuda.ExternalStream(handle)


def sync(stream):
    """wait for `stream` (a torch stream, a raw handle: that stream, not the whole device; None: the current stream)"""
    import torch
    (torch.cuda.current_stream() if stream is None else torch_stream(stream)).synchronize()


class Launch:
    """`with Launch(ref, stream) as L:` -- the launch context of a device-tier call.  Makes `ref`'s device current (no switch when it
    already is) and, when `stream` is a torch stream, that stream current, so that what `L.empty` / `L.scratch` allocate belongs to
    the launch stream and the caching allocator hands it out again only to work ordered after the kernels.  `L.sp` is the stream
    pointer for the fibd_* call.  Under a raw handle the allocator cannot know the stream: outputs are the caller's to order, and
    scratch, which is released when the call returns, is waited for on exit: the only wait the context adds (stream_device and
    stream_to_trk read their counts back and wait by design)."""

    def __init__(self, ref, stream=None):
        self.device, self.stream, self._ctx, self._wait = ref.device, stream, [], False

    def __enter__(self):
        import torch
        self._torch = torch
        if torch.cuda.current_device() != self.device.index:
            self._ctx.append(torch.cuda.device(self.device))
        if isinstance(self.stream, torch.cuda.Stream):
            self._ctx.append(torch.cuda.stream(self.stream))
        for c in self._ctx:
            c.__enter__()
        self.sp = stream_ptr(self.stream)
        return self

    def empty(self, shape, dtype):
        """an output tensor on the launch's device"""
        return self._torch.empty(shape, dtype=dtype, device=self.device)

    def scratch(self, nbytes):
        """8-byte aligned scratch of at least `nbytes` that lives until the call returns"""
        self._wait = self.stream is not None and not isinstance(self.stream, self._torch.cuda.Stream)
        return self._torch.empty((int(nbytes) + 7) // 8, dtype=self._torch.int64, device=self.device)

    def __exit__(self, *exc):
        try:
            if self._wait:
                sync(self.stream)
        finally:
            for c in reversed(self._ctx):
                c.__exit__(*exc)


def work(L, w, size, name, *args):
    """(scratch tensor, its bytes) for a call that needs size(*args) bytes: the caller's `w` checked (any dtype, 8-byte aligned, on
    the launch's device, large enough), or scratch of the launch `L` when the caller passed none.  `name` spells the need out."""
    need = size(*args)
    if w is None:
        return L.scratch(need), need
    nb = tensor(w, None, "work", ref=L).numel() * w.element_size()
    if nb < need or w.data_ptr() % 8:
        raise ArgError("work must be an 8-byte aligned CUDA tensor of at least %s = %d bytes" % (name, need))
    return w, nb


class Plan:
    """base of the plan classes: the native handle `_h` on one GPU (`device`), `close` and release on collection.  A subclass
    names its fib_*_plan_destroy entry in `_destroy` and fills `_h` in its __init__."""
    _destroy = None

    def __init__(self, device):
        self._h = C.c_void_p()
        self.device = device

    def close(self):
        if self._h:
            getattr(_lib.lib(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
