"""The one place where the Python wrapper decides how an array is read as a stack of images (api.image_stack_layout; the
six image operators call it through Context._image_stack): which axes are frames, rows, columns and channels, the pitch and
frame stride handed to the library, and whether the array passes through as it is or is made contiguous first.  Pure: numpy
only, no library, no GPU."""
import numpy as np
import pytest

from online_3d_reconstruction_amd.api import image_stack_layout


def base(*shape, dtype=np.uint8):
    return np.zeros(shape, dtype)


# name -> (array, single, F, rows, cols, ch, (pitch, fs) where the array passes through or None where it is copied)
COLOUR = {
    "grey contiguous": (base(5, 7), True, 1, 5, 7, 1, (7, 0)),
    "grey stack contiguous": (base(2, 5, 7), False, 2, 5, 7, 1, (7, 35)),
    "grey padded pitch": (base(5, 16)[:, :7], True, 1, 5, 7, 1, (16, 0)),
    "grey stack padded pitch and stride": (base(2, 8, 16)[:, :5, :7], False, 2, 5, 7, 1, (16, 128)),
    "B G R image": (base(5, 7, 3), True, 1, 5, 7, 3, (21, 0)),
    "three-pixel-wide grey stack reads as one B G R image": (base(4, 5, 3), True, 1, 4, 5, 3, (15, 0)),
    "B G R stack padded pitch": (base(2, 5, 10, 3)[:, :, :7], False, 2, 5, 7, 3, (30, 150)),
    "every other column": (base(5, 14)[:, ::2], True, 1, 5, 7, 1, None),
    "every other column of a stack": (base(2, 5, 14)[:, :, ::2], False, 2, 5, 7, 1, None),
    "frames reversed": (base(2, 5, 7)[::-1], False, 2, 5, 7, 1, None),
    "rows reversed": (base(5, 7)[::-1], True, 1, 5, 7, 1, None),
    "Fortran order": (np.asfortranarray(base(5, 7)), True, 1, 5, 7, 1, None),
    "Fortran order stack": (np.asfortranarray(base(2, 5, 7)), False, 2, 5, 7, 1, None),
    "one frame broadcast over the frame axis": (np.broadcast_to(base(5, 7), (4, 5, 7)), False, 4, 5, 7, 1, None),
    "three of four channels": (base(5, 7, 4)[..., :3], True, 1, 5, 7, 3, None),
    "three of four channels of a stack": (base(2, 5, 7, 4)[..., :3], False, 2, 5, 7, 3, None),
    "rows overlapping": (np.lib.stride_tricks.as_strided(base(64), (5, 7), (6, 1)), True, 1, 5, 7, 1, None),
    "frames overlapping": (np.lib.stride_tricks.as_strided(base(128), (2, 5, 7), (34, 7, 1)), False, 2, 5, 7, 1, None),
}
ELEMENTS = {
    "uint16 padded pitch": (base(5, 16, dtype=np.uint16)[:, :7], True, 1, 5, 7, 1, (32, 0)),
    "float64 stack contiguous": (base(3, 5, 7, dtype=np.float64), False, 3, 5, 7, 1, (56, 280)),
    "uint16 stack padded pitch and stride": (base(2, 8, 16, dtype=np.uint16)[:, :5, :7], False, 2, 5, 7, 1, (32, 256)),
    "a width of three is no colour axis": (base(4, 5, 3), False, 4, 5, 3, 1, (3, 15)),
    "uint16 every other column": (base(5, 14, dtype=np.uint16)[:, ::2], True, 1, 5, 7, 1, None),
    "float64 frames reversed": (base(3, 5, 7, dtype=np.float64)[::-1], False, 3, 5, 7, 1, None),
    "uint16 viewed at odd bytes": (np.lib.stride_tricks.as_strided(base(64, dtype=np.uint16), (5, 7), (14, 1)), True, 1, 5, 7, 1, None),
}
CASES = [(name, True) + c for name, c in COLOUR.items()] + [(name, False) + c for name, c in ELEMENTS.items()]


@pytest.mark.parametrize("name,colour,a,single,F,rows,cols,ch,through", CASES, ids=[c[0] for c in CASES])
def test_layout(name, colour, a, single, F, rows, cols, ch, through):
    E = a.itemsize
    lay = image_stack_layout(a.shape, a.strides, E, colour)
    assert (lay.single, lay.F, lay.rows, lay.cols, lay.ch) == (single, F, rows, cols, ch)
    assert lay.copy == (through is None)
    if through is None:  # what np.ascontiguousarray gives (a single image has no frame stride: 0 is passed)
        through = (cols * ch * E, 0 if single else rows * cols * ch * E)
        c = np.ascontiguousarray(a)
        assert c.strides[-3 if ch == 3 else -2] == through[0] and (single or c.strides[0] == through[1])
    assert (lay.pitch, lay.fs) == through
    # asked to be contiguous, every array is copied and has the copy's layout
    forced = image_stack_layout(a.shape, a.strides, E, colour, contiguous=True)
    assert forced.copy and forced[:5] == lay[:5] and forced.pitch == cols * ch * E and forced.fs == (0 if single else rows * forced.pitch)


def test_the_broadcast_stack_has_no_frame_stride():
    a = np.broadcast_to(base(5, 7), (4, 5, 7))
    assert a.strides[0] == 0 and image_stack_layout(a.shape, a.strides, 1, True).fs == 5 * 7


@pytest.mark.parametrize("colour,shape", [(False, (2, 3, 5, 7)), (False, (7,)), (True, (7,)), (True, (2, 2, 5, 7, 3))])
def test_other_ranks_are_refused(colour, shape):
    a = base(*shape)
    with pytest.raises(AssertionError):
        image_stack_layout(a.shape, a.strides, 1, colour)


def test_the_method_applies_it_to_numpy_arrays():
    """Context._image_stack on the host: the array handed on is the input itself where it passes through, a contiguous copy
    otherwise, and the address is that array's"""
    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib as L
    pad = base(2, 8, 16)[:, :5, :7]
    x, lay, addr, mem = o3dr.Context._image_stack(pad, colour=True)
    assert x is pad and not lay.copy and addr == pad.ctypes.data and mem == L.MEM_HOST
    rev = np.arange(70, dtype=np.uint8).reshape(2, 5, 7)[::-1]
    x, lay, addr, mem = o3dr.Context._image_stack(rev, colour=True)
    assert lay.copy and x.flags["C_CONTIGUOUS"] and np.array_equal(x, rev) and addr == x.ctypes.data and (lay.pitch, lay.fs) == (7, 35)
    x, lay, _, _ = o3dr.Context._image_stack(pad, colour=True, contiguous=True)
    assert lay.copy and x.flags["C_CONTIGUOUS"] and (lay.pitch, lay.fs) == (7, 35)
    x, lay, _, _ = o3dr.Context._image_stack([[1, 2], [3, 4]], colour=False)  # (anything np.asarray takes)
    assert (lay.rows, lay.cols, lay.pitch) == (2, 2, 2 * x.itemsize)
