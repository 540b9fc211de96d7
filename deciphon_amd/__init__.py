"""deciphon_amd -- MI355X-native Viterbi scan path of Deciphon.

The package is a thin ctypes binding over `lib/libdeciphon_hip.so` (HIP kernels for
gfx950 + the C ABI of `include/deciphon_hip.h`).  There is no CPU implementation
behind it: importing works anywhere, computing needs the built library and a GPU.
"""
from .press import DeciphonError, Press
from .hip import Engine, HipError, Window, device_count, encode, error_string, library_path, load_library, xtrans
from .scan import hit_on_read

__all__ = ["DeciphonError", "Engine", "HipError", "Window", "device_count", "encode", "error_string", "library_path",
           "load_library", "Press", "xtrans", "hit_on_read"]
