"""The three kernels that turn a waveform into encoder input - resample_sinc_kernel, logmel_kernel (csrc/audio.hip) and
melspec_db_kernel (csrc/clap_audio.hip) - held element by element to the bounds of tests/opcheck.py at their edge shapes.

Every case: the output goes into an opcheck.guarded buffer (NaN interior: an unwritten element fails; guard rows before and after
are compared bit for bit), the input is a view inside a larger buffer whose surroundings hold NaN (a read outside the clips
poisons an output), and a clip run alone must give the bits of its rows in the batched call (all three kernels are deterministic
per workgroup).  The operands and their reasons are stated in opcheck.py (RESAMPLE_CASES, logmel_case, DBMEL_CASES); the fp32 CPU
emulations of test_opcheck_cpu.py have met the same bounds on the same operands."""
import pytest
import torch

import clap_ref as R
import opcheck as oc
from conftest import record_parity, rel_err
from foley_amd.host import clap_score as CS, runtime as rt, sync_score as S

pytestmark = pytest.mark.gpu
LEFT_OUT_CAP = 1e-3          # no case may leave more than 0.1 % of its elements out of the per-element check
NAN = float("nan")


def _framed(x, dev, pad=2048):
    """x [B, N] as a contiguous view inside a larger device buffer whose surroundings hold NaN."""
    B, N = x.shape
    buf = torch.full((2 * pad + B * N,), NAN, device=dev, dtype=x.dtype)
    v = buf[pad:pad + B * N].view(B, N)
    v.copy_(x)
    return v


def _interior_untouched(g, what):
    torch.cuda.synchronize()
    g.check(what)
    assert bool(torch.isnan(g.view).all()), f"{what}: a refused call wrote into its output"


# ----------------------------------------------------------------------------- resampler
@pytest.mark.parametrize("name", list(oc.RESAMPLE_CASES))
def test_resample_sinc_elementwise(dev, name):
    x, taps, orig, new, width = oc.resample_case(name)
    ref, bound = oc.resample_ref_and_bound(x, taps, orig, new, width)
    B, n_out = ref.shape
    td = _framed(taps, dev)
    g = oc.guarded((B, n_out), torch.float32, dev)
    rt.op_resample_sinc(_framed(x, dev), orig, new, td, width, out=g.view)
    torch.cuda.synchronize()
    g.check(f"resample {name}")
    got = g.view.clone()
    worst = oc.assert_elementwise(got, ref, bound, f"resample {name}")
    for b in range(B if B > 1 else 0):
        ga = oc.guarded((1, n_out), torch.float32, dev)
        rt.op_resample_sinc(_framed(x[b:b + 1], dev), orig, new, td, width, out=ga.view)
        torch.cuda.synchronize()
        ga.check(f"resample {name} clip {b} alone")
        oc.assert_bits_equal(ga.view, got[b:b + 1], f"resample {name}: clip {b} alone against the batch")
    print(f"resample {name}: {orig}:{new}, {taps.shape[1]} taps, N {x.shape[1]} -> {n_out}: err / bound {worst:.3g}")
    record_parity(f"front_resample_{name}", err_over_bound=worst, taps=taps.shape[1], n_out=n_out)


@pytest.mark.parametrize("name", ["3to1_two_blocks", "147to160"])
def test_resample_sinc_refusals(dev, name):
    """Nout one phase group (`new` outputs) beyond the resampled length, N = 0 and ntaps = 0 are errors and write nothing."""
    lib = rt.load_library()
    x, taps, orig, new, width = oc.resample_case(name)
    B, N = x.shape
    n_out = -(-N * new // orig)
    xd, td = _framed(x, dev), _framed(taps, dev)
    g = oc.guarded((B, n_out + new), torch.float32, dev)
    call = lambda n, ntaps, nout: lib.foley_op_resample_sinc(xd.data_ptr(), B, n, orig, new, td.data_ptr(), ntaps, width,
                                                             g.view.data_ptr(), nout, None)
    assert call(N, taps.shape[1], n_out + new) == -1
    assert b"Nout exceeds the resampled length" in lib.foley_last_error()
    assert call(0, taps.shape[1], n_out) == -1
    assert call(N, 0, n_out) == -1
    _interior_untouched(g, f"resample refusals {name}")


# ----------------------------------------------------------------------------- log-mel
def _logmel_run(w, tb, dev, dtype, with_mel, tail_from):
    """One guarded launch: w [B, N16] framed in NaN, the samples no segment covers (from tail_from on) overwritten with NaN."""
    B, N = w.shape
    G = B * S.num_audio_segments(N)
    wd = _framed(w, dev)
    wd[:, tail_from:] = NAN
    gp = oc.guarded((G * 72, 256), dtype, dev)
    gm = oc.guarded((G, 128, 66), torch.float32, dev) if with_mel else None
    rt.op_logmel(wd, tb["basis"], tb["mel_lo"], tb["mel_len"], tb["mel_w"], out=gp.view, mel_out=gm.view if with_mel else None)
    torch.cuda.synchronize()
    gp.check("log-mel patches")
    if with_mel:
        gm.check("log-mel spectrogram")
    return gp.view.clone(), (gm.view.clone() if with_mel else None)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", list(oc.LOGMEL_CASES))
def test_logmel_elementwise(dev, name, B):
    w = oc.logmel_case(name, B)
    N = w.shape[1]
    nseg = S.num_audio_segments(N)
    tail = (nseg - 1) * 5120 + 10240
    tbc = S.logmel_tables("cpu")
    tb = {k: v.to(dev) for k, v in tbc.items()}
    ref, bound, share, a_log, silent = oc.logmel_ref_and_bound(w, tbc, dev)
    assert share <= LEFT_OUT_CAP, share
    what = f"log-mel {name} B {B}"
    patches, mel = _logmel_run(w, tb, dev, torch.float32, True, tail)
    worst = oc.assert_elementwise(mel, ref, bound, what)           # channels 126 and 127, which no patch reads, included
    # the patch layout without a tolerance, the 16-bit forms, and the form without mel_out
    oc.assert_bits_equal(patches, mel.cpu().unfold(1, 16, 10).unfold(2, 16, 10).reshape(-1, 256), what + ": patches against mel_out")
    oc.assert_bits_equal(_logmel_run(w, tb, dev, torch.float32, False, tail)[0], patches, what + ": patches without mel_out")
    for dt in (torch.float16, torch.bfloat16):
        oc.assert_bits_equal(_logmel_run(w, tb, dev, dt, False, tail)[0], patches.to(dt), what + f": {dt} patches")
    # a frame whose 400 staged samples are all zero: ONE value, the floor, in all 128 channels (its distance from the fp64 floor
    # was held to the bound above) - a frame or reflect index one sample off reads noise of amplitude 0.1
    assert int(silent.sum()) >= 13
    floor = mel.cpu().transpose(1, 2)[:, :65][silent]              # [silent frames, 128]
    oc.assert_bits_equal(floor, floor[:1, :1].expand_as(floor).contiguous(), what + ": silent frames")
    # the diffuse gate: the whole-tensor norm against the same recipe run in fp32 on the CPU, reference against reference
    e_kernel = rel_err(mel, ref)
    e_fp32 = rel_err(oc.logmel_emulation(w, tbc, torch.float32)[0], ref)
    print(f"{what}: err / bound {worst:.3g}, a_log {a_log:.3e}, rel_err kernel {e_kernel:.3e} fp32 CPU {e_fp32:.3e}, left out {share:.2e}")
    record_parity(f"front_logmel_{name}_b{B}", err_over_bound=worst, a_log=a_log, left_out=share, rel_err_kernel=e_kernel,
                  rel_err_fp32_cpu=e_fp32, norm_ratio=e_kernel / e_fp32)
    assert e_kernel <= 4 * e_fp32, (e_kernel, e_fp32)
    for b in range(B if B > 1 else 0):
        pa, ma = _logmel_run(w[b:b + 1], tb, dev, torch.float32, True, tail)
        oc.assert_bits_equal(ma, mel[b * nseg:(b + 1) * nseg], what + f": clip {b} alone, spectrogram")
        oc.assert_bits_equal(pa, patches[b * nseg * 72:(b + 1) * nseg * 72], what + f": clip {b} alone, patches")


def test_logmel_refusal(dev):
    """One sample short of a segment is an error and writes nothing."""
    lib = rt.load_library()
    tb = S.logmel_tables(dev)
    wd = _framed(oc.logmel_case("s1", 1), dev)
    gp, gm = oc.guarded((72, 256), torch.float32, dev), oc.guarded((1, 128, 66), torch.float32, dev)
    rc = lib.foley_op_logmel(wd.data_ptr(), 1, 10239, tb["basis"].data_ptr(), tb["mel_lo"].data_ptr(), tb["mel_len"].data_ptr(),
                             tb["mel_w"].data_ptr(), tb["mel_w"].shape[1], gp.view.data_ptr(), rt.DT_F32, gm.view.data_ptr(), None)
    assert rc == -1 and b"10240-sample segment" in lib.foley_last_error()
    _interior_untouched(gp, "log-mel refusal, patches")
    _interior_untouched(gm, "log-mel refusal, spectrogram")
    with pytest.raises(rt.FoleyRuntimeError):
        rt.op_logmel(wd[:, :10239].contiguous(), tb["basis"], tb["mel_lo"], tb["mel_len"], tb["mel_w"])


# ----------------------------------------------------------------------------- dB-mel
@pytest.fixture(scope="module")
def db_tables(dev):
    ex = R.extractor()
    tbc = CS.melspec_tables("cpu", ex.frequency_min, ex.frequency_max)
    fb = CS.slaney_mel_tables(ex.frequency_min, ex.frequency_max)[0]
    return ex, tbc, {k: v.to(dev) for k, v in tbc.items()}, fb


def _dbmel_run(x, starts, tb, dev):
    g = oc.guarded((x.shape[0] * len(starts), 1001, 64), torch.float32, dev)
    rt.op_melspec_db(_framed(x, dev), torch.tensor(starts, dtype=torch.int32, device=dev), tb["basis"], tb["mel_lo"], tb["mel_len"],
                     tb["mel_w"], out=g.view)
    torch.cuda.synchronize()
    g.check("dB-mel")
    return g.view.clone()


@pytest.mark.parametrize("name", list(oc.DBMEL_CASES))
def test_melspec_db_elementwise(dev, db_tables, name):
    ex, tbc, tb, fb = db_tables
    x, starts, wins = oc.dbmel_case(name)
    B, N = x.shape
    W = len(starts)
    # the reference once per DISTINCT window (clamped starts repeat a window)
    keys = [(b, min(max(s, 0), max(N - 480000, 0))) for b in range(B) for s in starts]
    uniq = sorted(set(keys))
    sel, back = [keys.index(k) for k in uniq], [uniq.index(k) for k in keys]
    ref_u, bound_u, share, a_log10, amb_u = oc.dbmel_ref_and_bound(wins[sel], tbc, dev)
    assert share <= LEFT_OUT_CAP, share
    got = _dbmel_run(x, starts, tb, dev)
    what = f"dB-mel {name}"
    worst = oc.assert_dbmel(got, ref_u[back], oc.Bound(bound_u.e[back]), amb_u[back], what)
    for i, k in enumerate(keys):                                    # a clamped start carries the bits of the window it lands on
        oc.assert_bits_equal(got[i], got[keys.index(k)], what + f": window {i} against the first window at {k}")
    if B > 1 or W > 1:                                              # a clip / a window alone: the bits of its rows in the batched call
        for b in range(B):
            for i, s in enumerate(starts):
                oc.assert_bits_equal(_dbmel_run(x[b:b + 1], [s], tb, dev)[0], got[b * W + i], what + f": clip {b} window {i} alone")
    # recorded, not gated: the figure test_melspec_db_op gates for its own clips - the kernel's largest distance from the
    # extractor over the fp32 restatement's
    feats = R.extractor_features([wins[i] if N > 480000 else x[keys[i][0]] for i in sel], ex)[:, 0]
    d_ref = float((R.melspec_fp32(wins[sel], fb) - feats).abs().max())
    d_got = float((got.cpu()[sel] - feats).abs().max())
    print(f"{what}: err / bound {worst:.3g}, a_log10 {a_log10:.3e}, extractor distance kernel {d_got:.3e} restatement {d_ref:.3e} dB")
    record_parity(f"front_dbmel_{name}", err_over_bound=worst, a_log10=a_log10, left_out=share, kernel_db=d_got, restatement_db=d_ref,
                  extractor_ratio=d_got / d_ref)


def test_melspec_db_refusals(dev, db_tables):
    """A clip shorter than one frame, and two windows of a clip below ten seconds, are errors and write nothing."""
    lib = rt.load_library()
    _, _, tb, _ = db_tables
    xd = _framed(oc.dbmel_case("n1500")[0], dev)
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    g = oc.guarded((2, 1001, 64), torch.float32, dev)
    call = lambda n, n_win: lib.foley_op_melspec_db(xd.data_ptr(), 1, n, st.data_ptr(), n_win, tb["basis"].data_ptr(), tb["mel_lo"].data_ptr(),
                                                    tb["mel_len"].data_ptr(), tb["mel_w"].data_ptr(), tb["mel_w"].shape[1],
                                                    g.view.data_ptr(), None)
    assert call(1023, 1) == -1 and b"1024-sample frame" in lib.foley_last_error()
    assert call(1500, 2) == -1 and b"one window" in lib.foley_last_error()
    _interior_untouched(g, "dB-mel refusals")
    with pytest.raises(rt.FoleyRuntimeError):
        rt.op_melspec_db(xd[:, :1023].contiguous(), st[:1], tb["basis"], tb["mel_lo"], tb["mel_len"], tb["mel_w"])
    with pytest.raises(rt.FoleyRuntimeError):
        rt.op_melspec_db(xd, st, tb["basis"], tb["mel_lo"], tb["mel_len"], tb["mel_w"])
