"""CPU: how many convolution launches the data-gradient pair of a ResNet block takes (bts_conv3d_bwd_data_pair_launches, answered from
the plan the launch runs on).  The Winograd F(2x2x2,3x3x3) kernel forms the 1x1x1 term in its own output side -- one launch -- where
it does not split the contraction and the 1x1x1 call left over would have been the streaming kernel's; everywhere else behind a
Winograd kernel the term stays a launch of its own.  No GPU: the query returns before any HIP call."""
import pytest

SWITCHES = ('BTS_WINO', 'BTS_W3', 'BTS_W3_T', 'BTS_WINO_MIN_WGS', 'BTS_IGEMM_DSC_MIN', 'BTS_IGEMM_C2_MIN', 'BTS_IGEMM_K1S_MIN',
            'BTS_IGEMM_UPM_MIN', 'BTS_IGEMM_NOGNFUSE', 'BTS_IGEMM_NOPAIR')
BWD, K3S1, X2, W3 = 1, 1, 2, 27


@pytest.fixture(scope='module')
def L():
    import bts_amd  # noqa: F401
    from bts_amd._lib import lib
    return lib()


@pytest.fixture
def default_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def launches(L, n, d, h, w, c, aligned=15, ld2=None):
    """dense rows, c -> c channels, as much workspace as the call asks for"""
    return L._bts_conv3d_bwd_data_pair_launches(n, d, h, w, c, c, c, c, ld2 or c, 0, aligned, -1)


def test_large_unsplit_levels_take_one_launch(L, default_switches):
    assert launches(L, 1, 128, 128, 128, 32) == 1
    assert launches(L, 1, 64, 64, 64, 64) == 1
    assert launches(L, 1, 128, 128, 128, 32) == 1      # (the same answer twice)


def test_small_and_split_shapes_keep_two_launches(L, default_switches):
    assert launches(L, 1, 8, 8, 32, 32) == 2           # 2,048 voxels: below the streaming kernel's bound
    assert launches(L, 1, 16, 16, 16, 256) == 2        # the 3x3x3 gradient splits the contraction here


def test_switches_keep_their_meaning(L, default_switches):
    default_switches.setenv('BTS_W3', '0')
    assert launches(L, 1, 128, 128, 128, 32) == 2      # the F(2x2,3x3) x direct form leaves the 1x1x1 term over
    default_switches.delenv('BTS_W3')
    default_switches.setenv('BTS_IGEMM_NOPAIR', '1')
    assert launches(L, 1, 128, 128, 128, 32) == 2      # two calls
    default_switches.delenv('BTS_IGEMM_NOPAIR')
    assert launches(L, 1, 128, 128, 128, 32) == 1


def test_operands_the_kernel_cannot_read_keep_two_launches(L, default_switches):
    assert launches(L, 1, 128, 128, 128, 32, aligned=15 & ~4) == 2      # dy2 off its 16-byte boundary
    assert launches(L, 1, 128, 128, 128, 32, ld2=34) == 2               # rows of dy2 that are no multiple of 16 bytes
    assert launches(L, 1, 128, 128, 128, 32, ld2=48) == 1               # dy2 as a slab view


def test_the_kernel_query_still_names_w3(L, default_switches):
    assert L._bts_conv3d_kernel(BWD, K3S1, 1, 128, 128, 128, 32, 32, 32, 32, 0, X2, 32, 0, 15, -1) == W3
    assert L._bts_conv3d_kernel(BWD, K3S1, 1, 64, 64, 64, 64, 64, 64, 64, 0, X2, 64, 0, 15, -1) == W3
    assert L._bts_conv3d_kernel(BWD, K3S1, 1, 8, 8, 32, 32, 32, 32, 32, 0, X2, 32, 0, 15, -1) == 4      # 8 workgroups: the tiled kernel, M128 N32
