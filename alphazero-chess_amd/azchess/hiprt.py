"""The few calls of the HIP runtime libaz is bound to, through ctypes: device buffers, a stream and
events for callers of the device-pointer entry points (az_net_forward_device) -- tools and tests."""
import ctypes as C

from . import _lib as L


class Hip:
    def __init__(self):
        paths = L.hip_runtime_paths()
        if not paths:
            raise RuntimeError("libaz maps no HIP runtime")
        self.rt = C.CDLL(paths[0])

    def ck(self, rc):
        if rc != 0:
            raise RuntimeError("HIP error %d" % rc)

    def multiprocessor_count(self, device=0):
        """compute units of `device` (hipDeviceAttributeMultiprocessorCount = 63, hip_runtime_api.h)"""
        n = C.c_int()
        self.ck(self.rt.hipDeviceGetAttribute(C.byref(n), 63, device))
        return n.value

    def malloc(self, nbytes):
        p = C.c_void_p()
        self.ck(self.rt.hipMalloc(C.byref(p), C.c_size_t(nbytes)))
        return p

    def free(self, p):
        self.ck(self.rt.hipFree(p))

    def copy_in(self, p, arr):
        """host array -> the device buffer p (synchronous)"""
        self.ck(self.rt.hipMemcpy(p, arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes), 1))

    def upload(self, arr):
        p = self.malloc(arr.nbytes)
        self.copy_in(p, arr)
        return p

    def download(self, p, arr):
        self.ck(self.rt.hipMemcpy(arr.ctypes.data_as(C.c_void_p), p, C.c_size_t(arr.nbytes), 2))
        return arr

    def stream(self):
        s = C.c_void_p()
        self.ck(self.rt.hipStreamCreate(C.byref(s)))
        return s

    def stream_synchronize(self, s):
        self.ck(self.rt.hipStreamSynchronize(s))

    def stream_destroy(self, s):
        self.ck(self.rt.hipStreamDestroy(s))

    def event(self):
        e = C.c_void_p()
        self.ck(self.rt.hipEventCreate(C.byref(e)))
        return e

    def record(self, e, s):
        self.ck(self.rt.hipEventRecord(e, s))

    def elapsed_ms(self, e0, e1):
        self.ck(self.rt.hipEventSynchronize(e1))
        ms = C.c_float()
        self.ck(self.rt.hipEventElapsedTime(C.byref(ms), e0, e1))
        return float(ms.value)
