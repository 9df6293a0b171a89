"""The workspace sizes of the five re-ranking size functions, pinned to the
values of the build before the carve was unified (RrCarve), and
each call's capacity check tied to its own size function.  Without a GPU: a
size function is host arithmetic and the capacity check comes before the first
GPU call, so addresses that are never read stand in for the buffers.

SIZES and LD_SIZES were recorded from the library built at the commit before
RrCarve; they are literals, never recomputed from the code under test."""
import pytest

OK, INVALID_ARG, CAPACITY = 0, -1, -4
SYMMETRIC, WHOLE = 1, 2
BASE = 0x10000000                  # a 256-byte aligned address; nothing reads it
P = BASE


def _lib():
    from pps_amd import _lib
    return _lib.lib()


# (Q, G, k1, k2, pps_rerank_workspace_bytes, pps_rerank_rows_workspace_bytes,
#  pps_rerank_features_workspace_bytes at segments 0 and 3,
#  pps_rerank_prepared_workspace_bytes at segments 0 and 3)
SIZES = [
    (1, 21, 20, 6, 594176, 591872, 1382400, 1382400, 1389824, 1389824),
    (1, 21, 6, 3, 321280, 318976, 1106944, 1106944, 1109760, 1109760),
    (1, 21, 20, 1, 143616, 141312, 931840, 931840, 939264, 939264),
    (1, 650, 20, 6, 19159808, 17461760, 30482432, 30372864, 20936448, 20936448),
    (1, 650, 6, 3, 11087616, 9389568, 22118400, 22082048, 12645632, 12645632),
    (1, 650, 20, 1, 5827328, 4129280, 17149952, 17040384, 7603968, 7603968),
    (1, 17661, 20, 6, 1721621760, 473695488, 697042176, 683924224, 554949632, 554949632),
    (1, 17661, 6, 3, 1502612736, 254686464, 463353088, 458980608, 330006016, 330006016),
    (1, 17661, 20, 1, 1359904000, 111977728, 335324416, 322206464, 193231872, 193231872),
    (1, 38400, 20, 6, 6928925440, 1029917184, 1253263872, 1250597888, 1206557952, 1206557952),
    (1, 38400, 6, 3, 6452753152, 553744896, 762411520, 761523200, 717483264, 717483264),
    (1, 38400, 20, 1, 6142472960, 243464704, 466811392, 464145408, 420105472, 420105472),
    (5, 21, 20, 6, 701952, 698880, 1489920, 1489920, 1498368, 1498368),
    (5, 21, 6, 3, 379392, 376320, 1164288, 1164288, 1167616, 1167616),
    (5, 21, 20, 1, 169472, 166400, 957440, 957440, 965888, 965888),
    (5, 650, 20, 6, 19287552, 17568768, 30592000, 30481920, 21044480, 21044480),
    (5, 650, 6, 3, 11165696, 9446912, 22176768, 22139904, 12703488, 12703488),
    (5, 650, 20, 1, 5873152, 4154368, 17177600, 17067520, 7630080, 7630080),
    (5, 17661, 20, 6, 1722296064, 473804288, 697150976, 684034560, 555059968, 555059968),
    (5, 17661, 6, 3, 1503237888, 254746112, 463412736, 459040768, 330066176, 330066176),
    (5, 17661, 20, 1, 1360496384, 112004608, 335351296, 322234880, 193260288, 193260288),
    (5, 38400, 20, 6, 6930261248, 1030024192, 1253370880, 1250706944, 1206666496, 1206666496),
    (5, 38400, 6, 3, 6454039296, 553802240, 762468864, 761581056, 717541120, 717541120),
    (5, 38400, 20, 1, 6143726848, 243489792, 466836480, 464172544, 420132096, 420132096),
    (150, 21, 20, 6, 4705280, 4587520, 5403136, 5403136, 5458176, 5458176),
    (150, 21, 6, 3, 2584576, 2466816, 3262976, 3262976, 3282176, 3282176),
    (150, 21, 20, 1, 1203200, 1085440, 1901056, 1901056, 1956096, 1956096),
    (150, 650, 20, 6, 24017408, 21457408, 41790464, 41521664, 24982272, 24982272),
    (150, 650, 6, 3, 14097408, 11537408, 31422464, 31332864, 14810368, 14810368),
    (150, 650, 20, 1, 7633408, 5073408, 25406464, 25137664, 8598272, 8598272),
    (150, 17661, 20, 6, 1746691072, 477692928, 701039616, 687996416, 558997760, 558997760),
    (150, 17661, 6, 3, 1525834752, 256836608, 465503232, 461155840, 332173568, 332173568),
    (150, 17661, 20, 1, 1381921792, 112923648, 336270336, 323227136, 194228480, 194228480),
    (150, 38400, 20, 6, 6978631424, 1033912832, 1257259520, 1254668800, 1210604288, 1210604288),
    (150, 38400, 6, 3, 6500611328, 555892736, 764559360, 763696128, 719648000, 719648000),
    (150, 38400, 20, 1, 6189127424, 244408832, 467755520, 465164800, 421100288, 421100288),
    (2228, 21, 20, 6, 80579072, 60320000, 178100480, 174699776, 178822656, 175454208),
    (2228, 21, 6, 3, 52691456, 32432384, 147190016, 146056448, 147437056, 146314240),
    (2228, 21, 20, 1, 34519552, 14260480, 132040960, 128640256, 132763136, 129394688),
    (2228, 650, 20, 6, 110343168, 77188608, 261388800, 255586816, 195902720, 192534272),
    (2228, 650, 6, 3, 74655744, 41501184, 220866048, 218932224, 156576512, 155453696),
    (2228, 650, 20, 1, 51401728, 18247168, 202447360, 196645376, 136961280, 133592832),
    (2228, 17661, 20, 6, 2115952128, 533424128, 756770816, 744775168, 763462912, 750344448),
    (2228, 17661, 6, 3, 1869328384, 286800384, 495467008, 491468800, 497703680, 493331200),
    (2228, 17661, 20, 1, 1708625408, 126097408, 349444096, 337448448, 356136192, 343017728),
    (2228, 38400, 20, 6, 7692181760, 1089644032, 1312990720, 1311447552, 1326651136, 1323984640),
    (2228, 38400, 6, 3, 7188394240, 585856512, 794523136, 794009088, 799082752, 798193920),
    (2228, 38400, 20, 1, 6860120320, 257582592, 480929280, 479386112, 494589696, 491923200),
]
LD_SIZES = [
    ('inplace', 2228, 17661, 'whole', (19892,), 20, 6, 0, 2115952128),
    ('inplace', 2228, 17661, 'whole', (19892,), 20, 6, 1, 690898944),
    ('inplace', 2228, 17661, 'whole', (19892,), 20, 6, 3, 533504000),
    ('short', 150, 650, 'whole', (800,), 20, 6, 0, 24017408),
    ('short', 150, 650, 'whole', (800,), 20, 6, 1, 24017408),
    ('short', 150, 650, 'whole', (800,), 20, 6, 3, 24017408),
    ('odd_ld', 2228, 17661, 'whole', (19889,), 20, 6, 0, 2115952128),
    ('odd_ld', 2228, 17661, 'whole', (19889,), 20, 6, 1, 2115952128),
    ('odd_ld', 2228, 17661, 'whole', (19889,), 20, 6, 3, 2115952128),
    ('inplace_sep', 2228, 17661, 'separate', (17664, 2228), 20, 6, 0, 2115952128),
    ('inplace_sep', 2228, 17661, 'separate', (17664, 2228), 20, 6, 1, 690898944),
    ('inplace_sep', 2228, 17661, 'separate', (17664, 2228), 6, 3, 1, 444275200),
    ('odd_ld_sep', 2228, 17661, 'separate', (17661, 2228), 20, 6, 1, 2115952128),
]


def _whole(Q, G, ld):
    """q_q, q_g, g_g as the blocks of one [N, ld] matrix (what PPS_RERANK_WHOLE
    requires): -> (q_g, ld_qg, q_q, ld_qq, g_g, ld_gg)."""
    return (BASE + 4 * Q, ld, BASE, ld, BASE + 4 * (Q * ld + Q), ld)


def _separate(Q, G, ldg, ldq):
    """Three buffers of their own, each 256-byte aligned."""
    qq = BASE
    qg = (BASE + 4 * Q * ldq + 256 + 255) & ~255
    gg = (qg + 4 * Q * ldg + 255) & ~255
    return (qg, ldg, qq, ldq, gg, ldg)


def _blocks(layout, Q, G, args):
    return _whole(Q, G, *args) if layout == 'whole' else _separate(Q, G, *args)


@pytest.mark.parametrize('row', SIZES, ids=lambda r: 'Q%d-G%d-k%d-%d' % r[:4])
def test_sizes_equal_the_recorded_ones(row):
    L = _lib()
    Q, G, k1, k2, dense, rows, feat0, feat3, prep0, prep3 = row
    assert L.pps_rerank_workspace_bytes(Q, G, k1, k2) == dense
    assert L.pps_rerank_rows_workspace_bytes(Q, G, k1, k2) == rows
    assert L.pps_rerank_features_workspace_bytes(Q, G, k1, k2, 0) == feat0
    assert L.pps_rerank_features_workspace_bytes(Q, G, k1, k2, 3) == feat3
    assert L.pps_rerank_prepared_workspace_bytes(Q, G, k1, k2, 0) == prep0
    assert L.pps_rerank_prepared_workspace_bytes(Q, G, k1, k2, 3) == prep3
    # flags 0 never takes the in-place size
    assert L.pps_rerank_workspace_bytes_ld(*_separate(Q, G, G, Q), Q, G, k1, k2, 0) == dense


@pytest.mark.parametrize('row', LD_SIZES, ids=lambda r: '%s-k%d-flags%d' % (r[0], r[5], r[7]))
def test_ld_sizes_equal_the_recorded_ones(row):
    name, Q, G, layout, args, k1, k2, flags, want = row
    got = _lib().pps_rerank_workspace_bytes_ld(*_blocks(layout, Q, G, args), Q, G, k1, k2, flags)
    assert got == want
    dense = _lib().pps_rerank_workspace_bytes(Q, G, k1, k2)
    in_place = name.startswith('inplace') and flags & SYMMETRIC
    assert (got < dense) if in_place else (got == dense)


def _capacity(name, args, ws_pos, need):
    """The call with need - 1 bytes: PPS_ERR_CAPACITY naming `need`."""
    L = _lib()
    assert need > 0
    args = list(args)
    args[ws_pos] = need - 1
    status = getattr(L, name)(*args)
    msg = L.pps_last_error().decode('utf-8')
    assert status == CAPACITY, (name, status, msg)
    assert msg.endswith('workspace too small: need %d bytes' % need), (name, msg)


@pytest.mark.parametrize('layout,Q,G,args,flags', [
    ('separate', 150, 650, (650, 150), 0),                       # dense
    ('separate', 150, 650, (650, 150), SYMMETRIC),               # dense: N < 16384
    ('whole', 2228, 17661, (19892,), SYMMETRIC | WHOLE),         # in place, q_g^T read in place
    ('separate', 2228, 17661, (17664, 2228), SYMMETRIC),         # in place with the q_g^T region
    ('whole', 2228, 17661, (19889,), SYMMETRIC | WHOLE),         # dense: ld % 4 != 0
])
def test_dense_call_checks_its_own_size(layout, Q, G, args, flags):
    L = _lib()
    blocks = _blocks(layout, Q, G, args)
    need = L.pps_rerank_workspace_bytes_ld(*blocks, Q, G, 20, 6, flags)
    in_place = flags & SYMMETRIC and Q + G >= 16384 and args[0] % 4 == 0
    assert (need < L.pps_rerank_workspace_bytes(Q, G, 20, 6)) == bool(in_place)
    _capacity('pps_re_ranking_ld', blocks + (Q, G, 20, 6, 0.3, flags, P, 0, P, None), 13, need)


@pytest.mark.parametrize('Q,G,k1,k2', [(150, 650, 20, 6), (5, 37, 6, 3), (5, 650, 20, 1)])
def test_row_form_calls_check_their_own_sizes(Q, G, k1, k2):
    L = _lib()
    _capacity('pps_re_ranking_rows', (P, Q + G, Q, G, k1, k2, 0.3, 0, P, 0, P, None), 9,
              L.pps_rerank_rows_workspace_bytes(Q, G, k1, k2))
    for seg in (0, 3):
        _capacity('pps_re_ranking_features',
                  (P, P, P, P, P, P, Q, G, 64, 0, k1, k2, 0.3, seg, 0, 0, P, 0, P, None), 17,
                  L.pps_rerank_features_workspace_bytes(Q, G, k1, k2, seg))
        _capacity('pps_re_ranking_prepared',
                  (P, P, P, P, P, P, Q, G, 64, 0, P, P, k1 + 1, P, k1, k2, 0.3, seg, 0, 0, P, 0, P,
                   None), 21,
                  L.pps_rerank_prepared_workspace_bytes(Q, G, k1, k2, seg))
