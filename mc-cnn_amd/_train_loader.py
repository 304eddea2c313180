"""The ctypes loader that the training libraries share.  `_train_lib.py`, `_train_slow_lib.py`, `_train_mb_lib.py`,
`_train_mb_slow_lib.py`, `_train_depth_lib.py` and `_train_slow_depth_lib.py` each declare their library (file name, symbol prefix, ABI version, error class, signatures) and bind
`load`, `last_error` and `check` from one `Loader`.  There is NO fallback: if the HIP library is missing or fails to load,
`load()` raises."""
import ctypes as C
import os

vp, i, f, i64, sz, text = C.c_void_p, C.c_int, C.c_float, C.c_int64, C.c_size_t, C.c_char_p


class Loader:
    def __init__(self, file_name, prefix, abi_version, error, signatures):
        """signatures: {symbol: (restype, argtypes)} of every exported symbol; `<prefix>_version` and
        `<prefix>_last_error` are among them."""
        self.file_name, self.prefix, self.abi_version, self.error, self.signatures = file_name, prefix, abi_version, error, signatures
        self.path = os.path.join(os.path.dirname(os.path.abspath(__file__)), file_name)
        self._lib = None

    def load(self):
        if self._lib is not None:
            return self._lib
        if not os.path.exists(self.path):
            raise ImportError(
                "mc-cnn_amd: %s not found. Build it with `make -C mc-cnn_amd/csrc` (hipcc, gfx950) or "
                "`python -c 'import __graft_entry__ as g; g.build()'`. There is no CPU fallback." % self.path)
        lib = C.CDLL(self.path)
        for name, (restype, argtypes) in self.signatures.items():
            fn = getattr(lib, name)          # a missing symbol raises here
            fn.restype, fn.argtypes = restype, argtypes
        if getattr(lib, self.prefix + "_version")() != self.abi_version:
            raise ImportError("mc-cnn_amd: %s ABI version mismatch" % self.file_name)
        self._lib = lib
        return lib

    def last_error(self):
        msg = getattr(self.load(), self.prefix + "_last_error")()
        return msg.decode("utf-8", "replace") if msg else ""

    def check(self, rc, what):
        if rc != 0:
            raise self.error("%s failed (rc=%d): %s" % (what, rc, self.last_error()))
