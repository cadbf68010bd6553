"""zero_max_cells on the host side: the CLI flag and the C default (no GPU needed)."""
import ctypes as C


def test_cli_flag_default_and_value():
    import C3POa
    a = C3POa.parse_args(["-r", "x.fq", "-s", "s.fa"])
    assert a.zero_max_cells == 16777216 and a.zero is True
    assert C3POa.parse_args(["-r", "x.fq", "-s", "s.fa", "--zero-max-cells", "67108864"]).zero_max_cells == 67108864


def test_default_config_zero_max_cells():
    from c3poa_amd import _lib
    c = _lib.default_config()
    assert c.zero_max_cells == 16777216 == _lib.ZERO_MAX_CELLS
    assert c.zero == 1 and (c.slots_poa, c.slots_win, c.dang_band) == (0, 0, 128)
    assert (c.conk_match, c.conk_mismatch, c.conk_penalty, c.mdistcutoff) == (5, -4, 20, 500)
    assert (c.pol_match, c.pol_mismatch, c.pol_gap, c.pol_window, c.pol_q) == (3, -5, -4, 500, 5)
    names = [f[0] for f in _lib.Config._fields_]
    assert names[-2:] == ["zero", "zero_max_cells"]
    assert _lib.Config.zero_max_cells.offset % 8 == 0 and C.sizeof(_lib.Config) == _lib.Config.zero_max_cells.offset + 8
    assert _lib.default_config(zero_max_cells=1 << 26).zero_max_cells == 1 << 26
