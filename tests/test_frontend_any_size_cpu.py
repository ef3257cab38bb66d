"""The windowed raw-k-space transform of the front-end (cine_raw_window_ifft2c) and the line-length query, on the host: argument
validation before any launch and the workspace size.  Runs without a GPU, through the loaded library."""
import ctypes

from cine_hip import _lib

EINVAL, EWORKSPACE = -1, -3


def test_fft_line_supported_matches_the_documented_rule():
    L = _lib.lib()
    for n in (1, 200, 400, 405, 512):
        assert L.cine_fft_line_supported(n) == 1, n
    for n in (401, 416, 540, 768, 1024, 0, -3):
        assert L.cine_fft_line_supported(n) == 0, n


def test_raw_window_rejects_bad_arguments_before_any_launch():
    L = _lib.lib()
    fake = ctypes.c_void_p(0x1000)        # never dereferenced: every call below fails on the host
    other = ctypes.c_void_p(0x2000)
    ws = ctypes.c_void_p(0x3000)
    big = 1 << 40
    args = dict(t_in=4, nx=416, ny=208, c=3, t_out=2, cx=200, cy=200)

    def call(raw=fake, out=other, w=ws, nbytes=big, **kw):
        a = dict(args, **kw)
        return L.cine_raw_window_ifft2c(raw, out, w, nbytes, a["t_in"], a["nx"], a["ny"], a["c"], a["t_out"], a["cx"], a["cy"],
                                        1e6, None)

    assert call(raw=None) == EINVAL and b"null" in L.cine_last_error()
    assert call(out=None) == EINVAL
    assert call(w=None) == EINVAL
    assert call(out=fake) == EINVAL                                   # aliased
    assert call(cx=417) == EINVAL and b"Invalid shapes" in L.cine_last_error()
    assert call(cy=209) == EINVAL
    assert call(cx=0) == EINVAL
    assert call(t_out=5) == EINVAL
    assert call(t_out=0) == EINVAL
    assert call(c=0) == EINVAL
    need = L.cine_raw_window_ws_bytes(2, 416, 208, 3, 200, 200)
    assert call(nbytes=need - 1) == EWORKSPACE and b"workspace" in L.cine_last_error()


def test_raw_window_workspace_is_positive_and_grows_with_the_shape():
    L = _lib.lib()
    small = L.cine_raw_window_ws_bytes(15, 416, 208, 30, 200, 200)
    assert small > 0
    assert L.cine_raw_window_ws_bytes(15, 768, 384, 30, 200, 200) > small
    assert L.cine_raw_window_ws_bytes(25, 416, 208, 30, 200, 200) > small
    assert L.cine_raw_window_ws_bytes(15, 416, 208, 31, 200, 200) > small
    assert L.cine_raw_window_ws_bytes(1, 1, 1, 1, 1, 1) > 0
    # at least the two window matrices and the intermediate of the cheaper axis order
    nx, ny, c, t, cx, cy = 416, 208, 30, 15, 200, 200
    inter = min(t * cx * ny * c, t * nx * c * cy)
    assert small >= 8 * (cx * nx + cy * ny + inter)
    assert L.cine_raw_window_ws_bytes(15, 416, 208, 30, 417, 200) == 0          # invalid window
    assert L.cine_raw_window_ws_bytes(0, 416, 208, 30, 200, 200) == 0
