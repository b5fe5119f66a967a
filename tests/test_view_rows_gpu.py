"""view_store_rows of csrc/orl_view.h — the way from a wavefront's bit rows in LDS to its 8 envs' rows of 0/1 bytes that k_action_mask
and k_rmcsa_mask share — called directly (tests/csrc/view_rows.hip copies a caller-made LDS image into LDS and calls it) and compared,
== on every byte of the buffer, with a plain-loop reference: column r * cpp + s = bit s of row r, the reject column, the fallback,
pad columns 0, and the rows of the envs >= B left at the sentinel the buffer was filled with.  Shapes at the 16-column chunk, 32-bit
word and 64-slot word edges.  The non-gpu part checks the reference against hand-written rows and cross-compiles the harness."""
import ctypes as C
import functools
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "view_rows.hip")
SENTINEL = 0xA5

NROWS = (1, 5, 9)
CPP = (1, 6, 15, 16, 17, 31, 32, 33, 64, 65, 320)
SHAPES = [(n, c) for n in NROWS for c in CPP]
SHAPE_IDS = ["r%d_c%d" % s for s in SHAPES]
BATCHES = (1, 8, 9)  # a part wavefront, a whole one, a second one


# ---- the harness ------------------------------------------------------------------------------------------------------------
def harness_path():
    """tests/csrc/view_rows.hip compiled for gfx950 into the package's build directory, keyed as tests/test_row_prims.py keys its
    harness: the unit, the compiler's arguments, and _build.source_hash() — every file of csrc/ (orl_view.h among them), the
    library's flags, the compiler's version.  Libraries of other keys can never be loaded again and are dropped."""
    from optical_rl_gym_amd import _build

    args = _build.HIPCC_FLAGS + ["-I", _build.CSRC, "-shared"]
    with open(SRC, "rb") as f:
        key = hashlib.sha256(f.read() + " ".join(args).encode() + _build.source_hash().encode()).hexdigest()[:16]
    directory = os.path.join(_build.HERE, "build")
    out = os.path.join(directory, "view_rows_%s.so" % key)
    if not os.path.exists(out):
        os.makedirs(directory, exist_ok=True)
        tmp = out + ".tmp.%d" % os.getpid()
        subprocess.check_call([_build.hipcc_path()] + args + [SRC, "-o", tmp])
        os.replace(tmp, out)
    for name in os.listdir(directory):
        if name.startswith("view_rows_") and name.endswith(".so") and name != os.path.basename(out):
            os.unlink(os.path.join(directory, name))
    return out


@functools.lru_cache(maxsize=None)
def harness():
    from optical_rl_gym_amd import _lib

    _lib.lib()  # first: it brings in the one HIP runtime the process shares with PyTorch (a second copy would find no device)
    lib = C.CDLL(harness_path())
    lib.vr_store_rows.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_int]
    lib.vr_store_rows.restype = C.c_int
    return lib


# ---- the image and its reference ------------------------------------------------------------------------------------------------
def row_words(cpp):
    return (cpp + 31) // 32


def pitch_of(nrows, cpp):
    return (nrows * cpp + 1 + 15) // 16 * 16


def reference(image, nrows, cpp, allow, B, sentinel=SENTINEL):
    """image: uint32 [envs][nrows * rw + 2] (bit rows, pad word, flag word) -> uint8 [envs][pitch], plain loops"""
    rw, pitch = row_words(cpp), pitch_of(nrows, cpp)
    out = np.full((len(image), pitch), sentinel, np.uint8)
    for e in range(B):
        words = [int(w) for w in image[e]]
        fallback = not allow and words[nrows * rw + 1] == 0
        for col in range(pitch):
            out[e, col] = 0
        for r in range(nrows):
            for s in range(cpp):
                bit = (words[r * rw + (s >> 5)] >> (s & 31)) & 1
                out[e, r * cpp + s] = 1 if fallback else bit
        out[e, nrows * cpp] = 1 if allow else 0
    return out


def make_image(nrows, cpp, B, fill, seed):
    """envs padded to whole wavefronts; flag words mixed 0 and 1 across the envs (independent of the rows: the function under test
    takes the flag's word for it).  `random` fills every word at random, the bits of a row beyond its cpp columns and the pad word
    included: they must not reach the output."""
    rw = row_words(cpp)
    envs = (B + 7) // 8 * 8
    rng = np.random.RandomState(seed)
    if fill == "ones":
        image = np.full((envs, nrows * rw + 2), 0xFFFFFFFF, np.uint32)
    elif fill == "zeros":
        image = np.zeros((envs, nrows * rw + 2), np.uint32)
    else:
        image = rng.randint(0, 1 << 32, size=(envs, nrows * rw + 2), dtype=np.uint64).astype(np.uint32)
    image[:, nrows * rw + 1] = (np.arange(envs) * 5 // 3 + seed) % 2  # seed 0: 0 1 1 1 0 0 0 1 | 1 1 ...: both values in the first 8 envs
    if B == 1:
        image[0, nrows * rw + 1] = seed % 2
    return np.ascontiguousarray(image)


# ---- not gpu ----------------------------------------------------------------------------------------------------------------------
def test_reference_on_hand_written_rows():
    # 2 rows of 3 columns, one word each: rows 0b101 and 0b010 (bits beyond the 3 columns set in the word: not columns), flag 1
    img = np.array([[0b11101, 0b1010, 0xFFFFFFFF, 1]], np.uint32)
    assert reference(img, 2, 3, 1, 1).tolist() == [[1, 0, 1, 0, 1, 0, 1] + [0] * 9]
    assert reference(img, 2, 3, 0, 1).tolist() == [[1, 0, 1, 0, 1, 0, 0] + [0] * 9]
    # no provisioning column (flag 0): with rejection the bits as they are and the reject column, without it the fallback
    img = np.array([[0, 0, 0, 0]], np.uint32)
    assert reference(img, 2, 3, 1, 1).tolist() == [[0, 0, 0, 0, 0, 0, 1] + [0] * 9]
    assert reference(img, 2, 3, 0, 1).tolist() == [[1, 1, 1, 1, 1, 1, 0] + [0] * 9]
    # 1 row of 33 columns across a word edge (bits 0, 31, 32 set), pitch 48; a second env beyond B = 1 stays at the sentinel
    img = np.array([[(1 << 31) | 1, 1, 0, 1], [1, 0, 0, 1]], np.uint32)
    got = reference(img, 1, 33, 1, 1, sentinel=7)
    want = [0] * 48
    for c in (0, 31, 32, 33):
        want[c] = 1
    assert got.tolist() == [want, [7] * 48]
    # 16 columns: the reject column starts a chunk of its own
    assert pitch_of(1, 16) == 32 and pitch_of(5, 32) == 176 and pitch_of(1, 15) == 16
    assert reference(np.array([[0xFFFF, 0, 1]], np.uint32), 1, 16, 1, 1).tolist() == [[1] * 17 + [0] * 15]


def test_images_mix_the_flag_words():
    for nrows, cpp in SHAPES:
        for B in BATCHES:
            for seed in (0, 1):
                flags = make_image(nrows, cpp, B, "random", seed)[:B, -1]
                assert set(flags.tolist()) <= {0, 1} and (B == 1 or set(flags.tolist()) == {0, 1})
    assert {int(make_image(1, 1, 1, "zeros", s)[0, -1]) for s in (0, 1)} == {0, 1}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_harness_cross_compiles_for_gfx950():
    path = harness_path()
    assert os.path.exists(path) and os.path.getsize(path) > 0
    rel = os.path.relpath(path, ROOT)
    assert rel.startswith(os.path.join("optical_rl_gym_amd", "build")), rel  # git-ignored, and not under csrc/ (hashed by the build)
    with open(path, "rb") as f:
        blob = f.read()
    assert b"vr_store_rows" in blob and b"k_view_rows" in blob


def test_harness_key_follows_the_shared_header():
    """orl_view.h is one of the files _build.source_hash() reads: a change to it rebuilds the library and this harness."""
    from optical_rl_gym_amd import _build

    assert os.path.join(_build.CSRC, "orl_view.h") in [os.path.normpath(s) for s in _build.sources()]


# ---- gpu ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nrows,cpp", SHAPES, ids=SHAPE_IDS)
def test_bit_rows_to_byte_rows(nrows, cpp):
    rw, pitch = row_words(cpp), pitch_of(nrows, cpp)
    for B in BATCHES:
        for allow in (0, 1):
            for k, fill in enumerate(("ones", "zeros", "random")):
                seed = allow + k  # (both flag patterns meet both settings of allow_rejection)
                image = make_image(nrows, cpp, B, fill, seed)
                out = np.full((len(image), pitch), SENTINEL, np.uint8)
                rc = harness().vr_store_rows(image.ctypes.data, nrows, rw, cpp, allow, B, out.ctypes.data, pitch)
                assert rc == 0, "vr_store_rows: error %d" % rc
                want = reference(image, nrows, cpp, allow, B)
                bad = np.argwhere(out != want)
                assert len(bad) == 0, "nrows %d cpp %d B %d allow %d %s: %d bytes differ, first at env %d column %d: got %d, expected %d" % (
                    nrows, cpp, B, allow, fill, len(bad), bad[0][0], bad[0][1], out[tuple(bad[0])], want[tuple(bad[0])])
