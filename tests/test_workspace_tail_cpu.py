"""The layout behind the base workspace, without a GPU: tests/cabi/workspace_tail.cpp (g++, -Wall -Werror) includes
ief-vad_amd/csrc/workspace_tail.h -- the header every *_workspace_bytes query and both forward routes of libiefvad.so take their
sizes and places from -- and prints the offsets for each query.

The expected sizes below are worked out by hand, not printed by the code (nb = chunks of a pass, R = 256 nb rows):
  w_rows  2 R D 4 bytes          D=768: 1 572 864 nb    D=512: 1 048 576 nb     (present with w_rows or with the column sums)
  colsum  nb 2 D 8 bytes         D=768:    12 288 nb    D=512:     8 192 nb
  z_prev  R D 4 bytes            D=768:   786 432 nb    D=512:   524 288 nb
  var     V R (2 D + 1) 4 bytes  D=768: 1 573 888 nb V  D=512: 1 049 600 nb V
  smp     var with V = 4         D=768: 6 295 552 nb    D=512: 4 198 400 nb
in this order behind the base, 256 nb (14 D + 4) 4 + 256 bytes: D=768: 11 014 144 nb + 256, D=512: 7 344 128 nb + 256.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGIONS = ("w_rows", "colsum", "z_prev", "var", "smp")
PER_CHUNK = {768: {"base": 11014144, "w_rows": 1572864, "colsum": 12288, "z_prev": 786432, "var": 1573888, "smp": 6295552},
             512: {"base": 7344128, "w_rows": 1048576, "colsum": 8192, "z_prev": 524288, "var": 1049600, "smp": 4198400}}
SHAPES = [(D, nb) for D in (768, 512) for nb in (1, 3)]


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    if shutil.which("g++") is None or shutil.which("make") is None:
        pytest.skip("g++ / make not available")
    out = tmp_path_factory.mktemp("workspace_tail")
    exe = os.path.join(str(out), "workspace_tail")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cabi"), f"OUT={out}", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]

    def ask(D, nb, w_rows=0, colsum=0, traj=0, variants=0, samples=0):
        """the offsets of one query by region name, and the total"""
        base = PER_CHUNK[D]["base"] * nb + 256
        r = subprocess.run([exe], input=f"{base} {nb} {D} {w_rows} {colsum} {traj} {variants} {samples}\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        got = [int(v) for v in r.stdout.split()]
        assert len(got) == 6
        assert all(v % 16 == 0 for v in got), got          # every region starts, and the workspace ends, 16-byte aligned
        return base, dict(zip(REGIONS, got[:5])), got[5]
    return ask


@pytest.mark.parametrize("D,nb", SHAPES)
def test_nothing_asked_for_is_the_base(ask, D, nb):
    base, off, total = ask(D, nb)
    assert total == base and all(v == base for v in off.values())


@pytest.mark.parametrize("D,nb", SHAPES)
def test_each_region_alone_starts_at_the_base(ask, D, nb):
    size = PER_CHUNK[D]
    for region, query, bytes_ in (("w_rows", dict(w_rows=1), size["w_rows"] * nb),
                                  ("w_rows", dict(colsum=1), (size["w_rows"] + size["colsum"]) * nb),      # the sums need the weights' home
                                  ("z_prev", dict(traj=1), size["z_prev"] * nb),
                                  ("var", dict(variants=1), size["var"] * nb),
                                  ("var", dict(variants=3), size["var"] * nb * 3),
                                  ("var", dict(variants=4), size["var"] * nb * 4),
                                  ("smp", dict(samples=1), size["smp"] * nb)):
        base, off, total = ask(D, nb, **query)
        assert off[region] == base, (region, query)
        assert total == base + bytes_, (region, query)


@pytest.mark.parametrize("D,nb", SHAPES)
def test_column_sums_lie_behind_the_weight_rows(ask, D, nb):
    size = PER_CHUNK[D]
    for w_rows in (0, 1):
        base, off, total = ask(D, nb, w_rows=w_rows, colsum=1)
        assert off["w_rows"] == base and off["colsum"] == base + size["w_rows"] * nb
        assert total == base + (size["w_rows"] + size["colsum"]) * nb


@pytest.mark.parametrize("D,nb", SHAPES)
def test_all_regions_in_order_without_overlap(ask, D, nb):
    size = PER_CHUNK[D]
    base, off, total = ask(D, nb, w_rows=1, colsum=1, traj=1, variants=2, samples=1)
    at = base
    for region, bytes_ in (("w_rows", size["w_rows"] * nb), ("colsum", size["colsum"] * nb), ("z_prev", size["z_prev"] * nb),
                           ("var", size["var"] * nb * 2), ("smp", size["smp"] * nb)):
        assert off[region] == at, region
        at += bytes_
    assert total == at


def test_two_layouts_in_full_by_hand(ask):
    assert ask(768, 1, w_rows=1, colsum=1, traj=1, variants=2, samples=1) == \
        (11014400, {"w_rows": 11014400, "colsum": 12587264, "z_prev": 12599552, "var": 13385984, "smp": 16533760}, 22829312)
    assert ask(512, 3, traj=1, samples=1) == \
        (22032640, {"w_rows": 22032640, "colsum": 22032640, "z_prev": 22032640, "var": 23605504, "smp": 23605504}, 36200704)
