"""k_poly_rows on the MI355X: the XCD-local mapping of its workgroups (poly_xcd = 1) writes the bits of the mapping
piece = blockIdx.x (poly_xcd = 0).  Cases and rules: poly_xcd_common.py."""
import pytest

import poly_xcd_common as pc

pytestmark = pytest.mark.gpu
N = 1 << 16


@pytest.mark.parametrize("ncols", [N, N - 1, 12345, 40000])
@pytest.mark.parametrize("prec", [64, 32])
def test_both_mappings_write_the_same_bits(hip_library, prec, ncols):
    pc.assert_same_bits(hip_library, N, prec, pc.scales(N, pc.IDX), ncols, want=pc.WANT)


def test_two_plane_chunks(hip_library):
    """poly_chunk_mb = 1 and 1.9 MB of coefficient planes: two launches of the kernel per call, each a grid of its own."""
    idx = sorted(set(pc.IDX) | set(range(105, 117)))
    pc.assert_same_bits(hip_library, N, 64, pc.scales(N, idx), N - 1, want=pc.WANT, min_chunks=2, extra={"poly_chunk_mb": 1})


@pytest.mark.parametrize("prec", [64, 32])
def test_a_whole_group_and_a_short_one(hip_library, prec):
    """N = 2^18, 511 pieces per row in complex128 (a whole group of 256 and one of 255), 256 in complex64 (one whole group)."""
    n = 1 << 18
    pc.assert_same_bits(hip_library, n, prec, pc.scales(n, [112, 142, 154, 166, 202]), n - 1000,
                        want={(2048, 8), (512, 8), (256, 8), (256, 6), (256, 4)} if prec == 64 else None)


def test_the_flagship_shape(hip_library):
    """N = 2^20, K' = 256 ... 4096, 2048 pieces per row: eight whole groups."""
    n = 1 << 20
    pc.assert_same_bits(hip_library, n, 64, pc.scales(n, [120, 150, 165, 180, 200, 250]), n)
