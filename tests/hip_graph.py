"""Stream capture and graph replay for the GPU tests (tests/test_gpu_capture.py): ctypes on the HIP runtime that the library has already loaded into the process --
stream create / destroy, begin / end capture, instantiate, launch, synchronise, destroy.  Every HIP return code is checked.  After the first failed call the module is
BROKEN: every later call raises at once and nothing more is started on the GPU through it."""
import ctypes

THREAD_LOCAL, RELAXED = 1, 2            # hipStreamCaptureModeThreadLocal, hipStreamCaptureModeRelaxed
_rt = None
BROKEN = None


class HipGraphError(RuntimeError):
    pass


def runtime():
    """the libamdhip64 that is mapped into this process (the library under test linked it): the same runtime, the same device context"""
    global _rt
    if _rt is None:
        path = None
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    path = line.split()[-1]
                    break
        if path is None:
            raise HipGraphError("libamdhip64 is not loaded: load the library under test first")
        _rt = ctypes.CDLL(path)
        _rt.hipGetErrorString.restype = ctypes.c_char_p
        _rt.hipGetErrorString.argtypes = [ctypes.c_int]
        vp, pvp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)
        _rt.hipStreamCreate.argtypes = [pvp]
        _rt.hipStreamDestroy.argtypes = _rt.hipStreamSynchronize.argtypes = _rt.hipGraphDestroy.argtypes = _rt.hipGraphExecDestroy.argtypes = [vp]
        _rt.hipStreamBeginCapture.argtypes = [vp, ctypes.c_int]
        _rt.hipStreamEndCapture.argtypes = [vp, pvp]
        _rt.hipGraphInstantiate.argtypes = [pvp, vp, pvp, ctypes.c_char_p, ctypes.c_size_t]
        _rt.hipGraphLaunch.argtypes = [vp, vp]
        _rt.hipGraphGetNodes.argtypes = [vp, pvp, ctypes.POINTER(ctypes.c_size_t)]
    return _rt


def _chk(code, what):
    global BROKEN
    if code != 0:
        BROKEN = "%s failed with HIP error %d (%s)" % (what, code, runtime().hipGetErrorString(code).decode())
        raise HipGraphError(BROKEN)


def _call(name, *args):
    if BROKEN:
        raise HipGraphError("not started: earlier, " + BROKEN)
    _chk(getattr(runtime(), name)(*args), name)


def stream_create():
    s = ctypes.c_void_p()
    _call("hipStreamCreate", ctypes.byref(s))
    return s.value


def stream_destroy(s):
    _call("hipStreamDestroy", s)


def synchronize(s):
    _call("hipStreamSynchronize", s)


class Graph:
    """`with capture(stream, enqueue) as g: g.launch(); ...` -- enqueue() runs between begin and end capture on `stream`; a call that fails in there ends the capture
    before the error travels on, so that the stream is left usable.  nodes = what the graph holds."""

    def __init__(self, stream, enqueue, mode=THREAD_LOCAL):
        self.stream, self.graph, self.exe = stream, ctypes.c_void_p(), ctypes.c_void_p()
        _call("hipStreamBeginCapture", stream, mode)
        try:
            enqueue()
        except BaseException:
            runtime().hipStreamEndCapture(stream, ctypes.byref(self.graph))      # (its own code is not the finding)
            if self.graph.value:
                runtime().hipGraphDestroy(self.graph)
            raise
        _call("hipStreamEndCapture", stream, ctypes.byref(self.graph))
        n = ctypes.c_size_t(0)
        _call("hipGraphGetNodes", self.graph, None, ctypes.byref(n))
        self.nodes = n.value
        _call("hipGraphInstantiate", ctypes.byref(self.exe), self.graph, None, None, 0)

    def launch(self):
        _call("hipGraphLaunch", self.exe, self.stream)
        synchronize(self.stream)

    def close(self):
        if self.exe.value:
            _call("hipGraphExecDestroy", self.exe)
            self.exe = ctypes.c_void_p()
        if self.graph.value:
            _call("hipGraphDestroy", self.graph)
            self.graph = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        if not BROKEN:
            self.close()
