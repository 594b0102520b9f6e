"""The minimal WAV reader/writer used for the reference's cache files (no GPU)."""
import struct

import numpy as np
import pytest


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_float_wav_roundtrip(tmp_path, dt):
    from foo_dsp_bfir_amd import wavio
    x = np.random.default_rng(0).uniform(-1, 1, (1001, 3)).astype(dt)
    p = str(tmp_path / "a.wav")
    wavio.write_wav_float(p, x, 44100)
    raw = open(p, "rb").read()
    assert raw[:4] == b"RIFF" and raw[8:16] == b"WAVEfmt " and struct.unpack("<H", raw[20:22])[0] == 3
    y, rate = wavio.read_wav(p)
    assert rate == 44100 and y.dtype == dt and np.array_equal(x, y)


def test_reader_skips_unknown_chunks_and_reads_pcm16(tmp_path):
    from foo_dsp_bfir_amd import wavio
    pcm = np.array([[0, 16384], [-32768, 32767]], dtype="<i2")
    fmt = struct.pack("<HHIIHH", 1, 2, 8000, 8000 * 4, 4, 16)
    peak = b"PEAK" + struct.pack("<I", 8) + b"\x00" * 8            # libsndfile writes such chunks
    body = b"WAVE" + b"fmt " + struct.pack("<I", 16) + fmt + peak + b"data" + struct.pack("<I", pcm.nbytes) + pcm.tobytes()
    p = tmp_path / "b.wav"
    p.write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body)
    y, rate = wavio.read_wav(str(p))
    assert rate == 8000 and np.array_equal(y, pcm.astype(np.float32) / np.float32(32768.0))


def test_djb_hash_uses_signed_chars():
    from foo_dsp_bfir_amd.equalizer import djb_hash
    assert djb_hash(b"") == 5381 and djb_hash(b"a") == (5381 * 33 + 97) & 0xFFFFFFFF
    assert djb_hash(bytes([200])) == (5381 * 33 - 56) & 0xFFFFFFFF


# ---- pinned to the reference: DJBHash of brutefir/hash.c compiled in place -------------------------------------
# tests/golden/djb_hash_ref.json holds inputs and the values the reference's own function returned
# (tests/golden/make_hash_golden.py; oracle/Makefile target `ref`).  This is the one piece of the path whose
# reference implementation builds in this image, so it is the one place where parity is pinned to reference output.
def _hash_cases():
    import json
    import os
    p = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "djb_hash_ref.json")
    return json.load(open(p))["cases"]


def test_djb_hash_matches_the_reference_function():
    from foo_dsp_bfir_amd.equalizer import djb_hash
    cases = _hash_cases()
    assert len(cases) >= 15 and any(c["kind"] == "bands" for c in cases)
    for c in cases:
        assert djb_hash(bytes.fromhex(c["hex"])) == c["djb"], c["kind"]


def test_equalizer_cache_name_carries_the_reference_hash():
    """equalizer::make_filename (equalizer.cpp:152-180): eq-<hex hash of freq|mag|phase doubles>-<taps/2>-..."""
    from foo_dsp_bfir_amd.equalizer import Equalizer
    eq = Equalizer.__new__(Equalizer)                      # the name needs no device
    eq.taps, eq.realsize, eq.n_channels, eq.sampling_rate = 65536, 8, 2, 44100
    for c in _hash_cases():
        if c["kind"] == "bands" and "freq" in c:
            assert eq.make_filename(c["freq"], c["mag"], c["phase"]) == "eq-%x-32768-8-2-44100.wav" % c["djb"]


def test_cpp_mirror_hash_matches_the_reference_function(tmp_path, bfir):
    """The same for host/equalizer_hip.hpp (plain g++, no GPU call)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_hash_pin")
    libdir = os.path.dirname(bfir.library_path())
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(root, "tests", "cpp", "test_hash_pin.cpp"),
                    "-o", exe, "-L" + libdir, "-lbfir_hip", "-Wl,-rpath," + libdir], check=True)
    lines = "".join("%s %d\n" % (c["hex"] or "-", c["djb"]) for c in _hash_cases())
    p = subprocess.run([exe], input=lines, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "ALL OK" in p.stdout, p.stdout + p.stderr


def test_fixture_regenerates_from_the_reference_when_it_is_present():
    """Where build() found the reference sources it compiled their hash.c into oracle/_ref (oracle/Makefile `ref`):
    check the committed fixture against that library.  Skipped (not failed) where it was not built -- the reference
    does not travel."""
    import ctypes as C
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.join(root, "oracle", "_ref", "libref_hash.so")
    if not os.path.exists(so):
        pytest.skip("oracle/_ref/libref_hash.so not built: build() found no reference sources")
    lib = C.CDLL(so)
    lib.DJBHash.restype = C.c_uint
    lib.DJBHash.argtypes = [C.c_char_p, C.c_uint]
    for c in _hash_cases():
        data = bytes.fromhex(c["hex"])
        assert lib.DJBHash(data, len(data)) == c["djb"]
