"""`ganon-build --parse host|device` without a GPU: the switch's refusal and help text, and host/genome_chunks.hpp -- where a buffer of
genome text is cut into the chunks the device tokenises, and the letters of a record too short for the device's pieces -- as a
stand-alone program under AddressSanitizer and UBSan (nothing is preloaded)."""
import os
import subprocess

from test_build_cpu import BIN_BUILD

HERE = os.path.dirname(os.path.abspath(__file__))


def test_parse_mode_is_validated_before_any_device_call(tmp_path):
    inp = tmp_path / "in.tsv"
    inp.write_text("no_such_file.fna\n")
    out = str(tmp_path / "o.ibf")
    for value in ("bogus", "", "Device", "gpu"):
        p = subprocess.run([BIN_BUILD, "-i", str(inp), "-o", out, "--parse", value], capture_output=True, text=True)
        assert p.returncode == 2 and "--parse has to be host or device" in p.stderr and p.stdout == "" and not os.path.exists(out), (value, p.stderr)
        assert "HIP" not in p.stderr and "device (" not in p.stderr  # refused before the device count is asked for
    p = subprocess.run([BIN_BUILD, "-i", str(inp), "-o", out, "--parse=bogus", "--hibf", "--verbose"], capture_output=True, text=True)
    assert p.returncode == 2 and "--parse has to be host or device" in p.stderr
    p = subprocess.run([BIN_BUILD, "--parse"], capture_output=True, text=True)
    assert p.returncode == 1 and "missing an argument" in p.stderr


def test_help_lists_parse():
    p = subprocess.run([BIN_BUILD, "--help"], capture_output=True, text=True)
    assert p.returncode == 0 and "--parse arg" in p.stderr and "GANON_BUILD_PARSE_CHUNK" in p.stderr


def test_genome_chunks_under_sanitizers(tmp_path):
    exe = str(tmp_path / "genome_chunks_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "genome_chunks_driver.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "" and p.stdout.startswith("ok "), (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
