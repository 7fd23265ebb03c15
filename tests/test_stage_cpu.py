"""The staging unit without a GPU: decoder_stage.hip is built into the library by both builds; the layout of a batch buffer and
the tables of the one unpack or conversion launch, as the product builds them, hold on the CPU, under the sanitizers, in a program
of their own."""
import os
import subprocess

from conftest import ROOT


def test_the_staging_unit_is_built_by_both_builds():
    from adsbdec_amd import _build
    assert "decoder_stage.hip" in _build.HIP_SOURCES
    assert "decoder_stage.hip.o" in open(os.path.join(ROOT, "Makefile")).read()
    assert "decoder_flavour.hip" in _build.HIP_SOURCES
    assert "decoder_flavour.hip.o" in open(os.path.join(ROOT, "Makefile")).read()


def test_layout_and_tables_under_the_sanitizers(tmp_path):
    """csrc/stage_layout.hpp, packed12.h's unpack12_table and sample_format.h's convert_table compiled for the host with
    -fsanitize=address,undefined, a program of its own (tests/cpp/stage_layout.cpp): seeded capture lists with lengths 0, 1 .. 9, one of
    2^29 groups, and empty captures first, last and adjacent; offsets aligned, in order and without overlap, the total the last end;
    rows only for captures with groups, the closing row the total; the offsets adsb_batch_unpacked_copy answers from are the layout's."""
    exe = tmp_path / "stage_layout"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "stage_layout.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok: 132 lists"), p.stdout + p.stderr


def test_flavours_under_the_sanitizers(tmp_path):
    """csrc/flavour.hpp compiled for the host with -fsanitize=address,undefined, a program of its own (tests/cpp/flavour.cpp): for
    every flavour and the capture lengths of the GPU rows (and every length below 4200, and four near 2^31 and 2^32) the power-sample
    count and the elements that go into scratch against the rules written out per flavour in the program; alignment, groups of 8,
    kinds and conversion numbers; .on_host() and .at() change the alignment alone."""
    exe = tmp_path / "flavour"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "flavour.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok: 33672 checks of 8 flavours"), p.stdout + p.stderr
