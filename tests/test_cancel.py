"""CPU side of sdr_iq_cancel (successive interference cancellation on the ring): the NumPy statement the GPU tests hold the
device to (sydr_amd/signal/cancel.py) against the oracle -- the projection identity through orc.epl, the hull and the
records helper, the near-far scenario through the oracle's PCPS -- the margins every integer-ring case keeps from a
rounding tie and from a rail, and ChannelManager.searchBehindTracked against a fake engine."""
import numpy as np
import pytest

import cancel_cases as cc
from oracle import sydr_oracle as orc
from sydr_amd import _lib
from sydr_amd.engine import make_items
from sydr_amd.signal import cancel as cn


def _identity_limit(fmt, n, amp_sum, theta_max, y_max):
    """What the prompt of an item may be on the samples its own least-squares amplitude was cancelled from: cf64, a single
    channel: the derived per-sample bound times n; an integer ring with no rail hit: each component rounded by at most
    0.5, n * sqrt(2) / 2."""
    if fmt in cc.RAIL:
        return n * np.sqrt(2.0) / 2.0
    return cn.parity_bound(fmt, amp_sum, theta_max, y_max, 1) * n


def _prompts_after(x, fmt, items, code, fs, w0, cap):
    """Cancel one channel's items with the amplitudes of the oracle's prompts; -> (prompt magnitudes on the output, limits)."""
    amps = np.zeros((len(items), 2))
    W = len(x)
    offs = cn.window_offsets(items, w0, cap)
    for k, (it, off) in enumerate(zip(items, offs)):
        n = int(it["n_samples"])
        if n:
            p = orc.epl(x[off:off + n], orc.pad_code(code), fs, float(it["carrier_hz"]), float(it["rem_carrier"]),
                        float(it["rem_code"]), float(it["code_step"]), (0.0,))
            amps[k] = cn.amplitudes_from_prompts(np.array(p), n)
    res = cn.cancel_statement(x, fmt, [(items, amps, code)], fs, w0, cap)
    assert res.stats["clipped_components"] == 0 and res.stats["samples_written"] == W
    out = []
    for k, (it, off) in enumerate(zip(items, offs)):
        n = int(it["n_samples"])
        if not n:
            continue
        p = orc.epl(res.window[off:off + n], orc.pad_code(code), fs, float(it["carrier_hz"]), float(it["rem_carrier"]),
                    float(it["rem_code"]), float(it["code_step"]), (0.0,))
        amp_sum = float(np.abs(amps[k]).sum())
        theta_max = abs(float(it["carrier_hz"])) * 2 * np.pi * n / fs + abs(float(it["rem_carrier"]))
        out.append((np.hypot(*p), _identity_limit(fmt, n, amp_sum, theta_max, float(np.abs(x).max()) + amp_sum)))
    return out


@pytest.mark.parametrize("fmt", [3, 0, 1], ids=["cf64", "ci8", "ci16"])
def test_projection_identity_against_the_oracle(fmt):
    """prompt / n is the least-squares amplitude: orc.epl of the statement's output with the item's own parameters is zero
    to rounding (cf64) or to the rounding of the ring's integers.  `multi`: one channel of 4-period epochs on a ring of
    noise, the window offset by w0; and the near-far ring's strong signal."""
    c = cc.geometry("multi")
    x = cc.window_of(cc.to_complex(cc.ring_image("multi", fmt)), c["w0"], c["W"])
    got = _prompts_after(x, fmt, c["items"][0], cc.slot_code(c["slots"][0]), c["fs"], c["w0"], c["capacity"])
    if fmt in (0, 3):
        nf = cc.near_far(fmt)
        got += _prompts_after(cc.to_complex(nf["image"]), fmt, nf["items"][0], cc.slot_code(nf["slots"][0]), cc.NEAR_FAR["fs"], 0, None)
    for mag, limit in got:
        print(f"{cc.FMT_NAMES[fmt]}: |prompt| {mag:.3e}, limit {limit:.3e} ({mag / limit:.3f})")
        assert mag <= limit
    assert len(got) >= 2


def test_amplitudes_from_prompts_and_padding():
    p = np.array([[[8000.0, -4000.0], [5.0, 5.0]]])
    a = cn.amplitudes_from_prompts(p, np.array([[4000, 0]]))
    assert a.tolist() == [[[2.0, -1.0], [0.0, 0.0]]]


def test_hull_and_items_from_records():
    rec = np.zeros((2, 3), dtype=_lib.TRACK_EPOCH_DTYPE)
    rec["start_sample"] = [[100, 4100, 8100], [2500, 6499, 0]]
    rec["n_samples"] = [[4000, 4000, 4001], [3999, 4000, 0]]            # the second channel ran two epochs: padding
    rec["carrier_hz_in"], rec["rem_carrier_in"], rec["rem_code_in"], rec["code_step_in"] = 1500.0, 0.25, 0.5, 0.25575
    rec["carrier_hz"] = 9999.0                                           # (the loop's OUTPUT: not what the epoch ran with)
    rec["corr"][..., 2:4] = [[[4000.0, 8000.0]] * 3, [[-3999.0, 0.0], [2000.0, 2000.0], [7.0, 7.0]]]
    items, amps, (w0, W) = cn.items_from_records(rec, [4, 9])
    assert (w0, W) == (100, 12101 - 100)
    assert items.shape == (2, 3) and items.dtype == _lib.EPL_ITEM_DTYPE
    assert items["code_slot"].tolist() == [[4, 4, 4], [9, 9, 9]]
    for dst, src in (("n_samples", "n_samples"), ("start_sample", "start_sample"), ("carrier_hz", "carrier_hz_in"),
                     ("rem_carrier", "rem_carrier_in"), ("rem_code", "rem_code_in"), ("code_step", "code_step_in")):
        assert np.array_equal(items[dst], rec[src])
    assert amps[0].tolist() == [[1.0, 2.0], [1.0, 2.0], [4000.0 / 4001, 8000.0 / 4001]]
    assert amps[1].tolist() == [[-1.0, 0.0], [0.5, 0.5], [0.0, 0.0]]
    assert cn.hull(items) == (100, 12001)
    with pytest.raises(ValueError):
        cn.hull(items[1:, 2:])
    # five taps: the centre is the third
    rec["corr"][..., 4:6] = 4000.0
    assert cn.items_from_records(rec[0], [0], n_taps=5)[1][0, 0].tolist() == [1.0, 1.0]


def test_the_statement_skips_padding_and_refuses_what_the_call_refuses():
    c = cc.geometry("short")
    res, image = cc.statement("short", 3)
    amps = cc.amps_of("short", 3)
    assert (c["items"]["n_samples"][1, 37:] == 0).all() and (c["items"]["n_samples"][3, 37:] == 0).all()
    live = c["items"]["n_samples"] > 0
    covered = np.zeros(c["W"], dtype=bool)
    for it in c["items"][live]:
        off = int(it["start_sample"]) - c["w0"]
        covered[off:off + int(it["n_samples"])] = True
    assert np.array_equal(covered, res.covered) and res.stats["samples_changed"] == covered.sum() < c["W"]
    win = cc.window_of(cc.to_complex(image), c["w0"], c["W"])
    assert np.array_equal(res.window[~covered], win[~covered])
    chans = cc.channels_of("short", amps)
    with pytest.raises(ValueError):
        cn.cancel_statement(win[:-100], 3, chans, c["fs"], c["w0"], c["capacity"])
    swapped = c["items"][0].copy()
    swapped[[2, 3]] = swapped[[3, 2]]
    with pytest.raises(ValueError):
        cn.cancel_statement(win, 3, [(swapped, amps[0], chans[0][2])], c["fs"], c["w0"], c["capacity"])
    with pytest.raises(ValueError):
        cn.cancel_statement(win, 3, chans * 17, c["fs"], c["w0"], c["capacity"])


def test_the_statement_across_the_rings_end_and_a_negative_chip_index():
    c = cc.geometry("stagger")
    assert c["w0"] + c["W"] > c["capacity"]
    offs = cn.window_offsets(c["items"], c["w0"], c["capacity"])
    assert offs.min() == 100 and (offs + c["items"]["n_samples"]).max() == c["W"] - 100
    m = cc.geometry("multi")["items"][0, 0]
    idx = orc.epl_indices(int(m["n_samples"]), float(m["rem_code"]), float(m["code_step"]), 0.0)
    assert idx[0] == 0 and idx.max() >= 4 * 1023
    # the replica is the oracle's: chip * conj(exp(1j * theta)) scaled by A
    code = orc.gold_code(19)
    r_re, r_im, theta = cn.replica(m, (cc.PHI, -1.0), code, 4e6)
    want = (cc.PHI - 1.0j) * code[(idx - 1) % 1023] * np.conj(np.exp(1j * theta))
    assert np.abs(r_re + 1j * r_im - want).max() < 1e-14


@pytest.mark.parametrize("fmt", [0, 1], ids=["ci8", "ci16"])
@pytest.mark.parametrize("name", cc.CASES)
def test_integer_cases_keep_clear_of_ties_and_rails(name, fmt):
    tie, rail = cc.tie_and_rail_margins(name, fmt)
    d = cc.bound(name, fmt)
    print(f"{name} {cc.FMT_NAMES[fmt]}: tie margin {tie:.3e}, rail margin {rail:.3e}, bound {d:.3e}")
    assert tie > d and rail > d
    assert cc.statement(name, fmt)[0].stats["clipped_components"] == 0


def test_the_rails_case_clips_and_keeps_clear_of_ties():
    tie, rail = cc.tie_and_rail_margins("stagger", 0, cc.RAIL_SCALE)
    d = cc.bound("stagger", 0, cc.RAIL_SCALE)
    res, _ = cc.statement("stagger", 0, cc.RAIL_SCALE)
    assert tie > d and rail > d and res.stats["clipped_components"] > 0
    assert np.abs(res.window.real).max() == 127.0 and np.abs(res.pre.real).max() > 127.5


@pytest.mark.parametrize("fmt", [3, 0], ids=["cf64", "ci8"])
def test_near_far_on_the_statement(fmt):
    """The precondition of the GPU test: with A 30 times B (29.5 dB, under the C/A isolation) the oracle's PCPS for B on the
    original samples returns a cross-correlation peak of A, on the statement's cancelled samples B's bin and code phase;
    the absent C's ratio drops."""
    nf, exp = cc.near_far(fmt), cc.near_far_expected(fmt)
    truth = list(nf["truth"])
    print(f"{cc.FMT_NAMES[fmt]}: truth {truth}; B before {exp['before_b']}, after {exp['after_b']}; C before {exp['before_c']}, "
          f"after {exp['after_c']}")
    assert exp["before_b"][0] != truth and exp["after_b"][0] == truth
    assert exp["after_b"][1] > 5.0 > exp["before_b"][1]
    assert exp["after_c"][1] < exp["before_c"][1]
    if fmt == 0:
        x = cc.to_complex(nf["image"])
        assert 85 < np.abs(x.real).max() <= 127 and exp["stats"]["clipped_components"] == 0
    assert np.abs(exp["amps"] - nf["amps_truth"]).max() < 0.03 * cc.NEAR_FAR_AMP[fmt]


# ------------------------------------------------------------------------------------------------ the manager's method
from fake_engine import OracleBank, OracleEngine  # noqa: E402
from sydr_amd.channel.l1ca_kaplan import ChannelL1CA_Kaplan  # noqa: E402
from sydr_amd.channel.manager import ChannelManager  # noqa: E402
from sydr_amd.utils.enumerations import ChannelState  # noqa: E402
from test_host_layer import KAPLAN_INI, channel_config, drive, rf_signal  # noqa: E402


class CancelEngine(OracleEngine):
    """OracleEngine + iq_cancel through the statement; keeps what it was handed and the records its bank's steps returned."""
    device_id = 0

    def __init__(self):
        super().__init__()
        self.cancel_calls, self.step_log, self.closed = [], [], False

    def bank(self, max_channels):
        bank, log = OracleBank(self, max_channels), self.step_log

        def step(channels, n_epochs=1, **kw):
            out = OracleBank.step(bank, channels, n_epochs, **kw)
            log.append((list(channels), out[0].copy(), out[2].copy()))
            return out
        bank.step = step
        self.bank_calls = bank.calls
        return bank

    def close(self):
        self.closed = True

    def iq_cancel(self, items, amps=None, fs=None, window=None, dst=None, dst_offset=0):
        self.cancel_calls.append(dict(items=np.array(items), amps=np.array(amps), fs=fs, window=window, dst=dst, dst_offset=dst_offset))
        w0, W = window
        win = self._complex(w0, W)
        chans = [(its, am, self.codes[int(its["code_slot"][0])]) for its, am in zip(items, amps)]
        res = cn.cancel_statement(win, self.iq_fmt, chans, fs, w0, self.iq_capacity)
        (self if dst is None else dst).iq_upload(cc.to_image(res.window, self.iq_fmt), w0 if dst is None else dst_offset)
        return res.stats


MGR_SATS = [dict(prn=9, doppler=2250.0, code_phase=417.3, phase=0.2, amp=75.0), dict(prn=23, doppler=-1250.0, code_phase=100.6, phase=0.7, amp=3.0)]


def _manager_pair():
    raw = orc.synth_iq(4e6, 41 * 4000, MGR_SATS, 1.0, 20260606)
    out = []
    for _ in range(2):
        eng = CancelEngine()
        mgr = ChannelManager(rf_signal(4e6), engine=eng)
        mgr.addChannel(ChannelL1CA_Kaplan, channel_config(KAPLAN_INI), 2)
        ch = mgr.requestTracking(9)
        drive(mgr, raw, 4000, 16)
        assert ch.channelState is ChannelState.TRACKING
        mgr.addNewRFData(raw[2 * 16 * 4000:])          # 25 ms more (a divisor of the ring), resident before the block
        out.append((eng, mgr, ch))
    return out


def _plain(p):
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in dict(p).items()}


def test_manager_searches_behind_the_tracked_channel():
    (eng1, twin, _), (eng2, mgr, ch) = _manager_pair()
    made = []
    mgr._make_search_engine = lambda: made.append(CancelEngine()) or made[-1]
    search = dict(doppler_range=5000.0, doppler_step=250.0, coh=1, noncoh=5)
    want_packets = [_plain(p) for p in twin.runBlock(24)]
    packets, rows = mgr.searchBehindTracked([23, 30], 24, search)
    assert [_plain(p) for p in packets] == want_packets and len(want_packets) == 25
    # what went down: the block's records, field by field, and the centre tap over n_samples
    assert len(eng2.cancel_calls) == 1 and len(made) == 1
    call = eng2.cancel_calls[0]
    members, rec, done = eng2.step_log[-1]
    assert members == [ch.channelID] and done[0] == 24
    items, amps = call["items"], call["amps"]
    assert items.shape == (1, 24) and (items["code_slot"] == ch.codeSlot).all()
    for dst, src in (("n_samples", "n_samples"), ("start_sample", "start_sample"), ("carrier_hz", "carrier_hz_in"),
                     ("rem_carrier", "rem_carrier_in"), ("rem_code", "rem_code_in"), ("code_step", "code_step_in")):
        assert np.array_equal(items[dst][0], rec[src][0])
    assert np.array_equal(amps[0], rec["corr"][0][:, 2:4] / rec["n_samples"][0][:, None])
    w0 = int(rec["start_sample"][0, 0])
    assert call["window"] == (w0, int(rec["n_samples"][0].sum())) and call["dst"] is made[0] and call["dst_offset"] == w0 % eng2.iq_capacity
    # the tracked ring is as the twin's; the search ring holds the residue, in which B is where the truth puts it
    assert np.array_equal(eng2.ring, eng1.ring)
    step_b = orc.CODE_RATE * (1 + MGR_SATS[1]["doppler"] / cc.L1) / 4e6
    left = (-(MGR_SATS[1]["code_phase"] + w0 * step_b)) % 1023
    assert (rows[0]["satelliteID"], rows[0]["peak_bin"], rows[0]["peak_code"]) == (23, 25, int(np.ceil(left * 4e6 / orc.CODE_RATE)))
    assert rows[0]["doppler_hz"] == -1250.0 and rows[0]["start_sample"] == w0
    assert rows[0]["peak_ratio"] > 1.8 > rows[1]["peak_ratio"] and rows[1]["satelliteID"] == 30
    eng2.load_gps_code(1, 23)
    before = eng2.pcps([1], w0, 4e6, 0.0, 5000.0, 250.0, 1, 5)
    assert [int(before[0][0]), int(before[1][0])] != [rows[0]["peak_bin"], rows[0]["peak_code"]]     # not without cancelling
    assert all(c.channelState is not ChannelState.TRACKING for c in mgr.channels.values() if c is not ch)   # it started none
    # a span shorter than the search needs; a C/N0 nobody reaches
    with pytest.raises(ValueError, match="needs"):
        mgr.searchBehindTracked([23], 2, search)
    with pytest.raises(ValueError, match="dB-Hz"):
        mgr.searchBehindTracked([23], 2, search, minCn0=99.0)
    assert len(eng2.cancel_calls) == 1
    mgr.close()
    twin.close()
    assert made[0].closed
