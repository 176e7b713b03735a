"""Monte-Carlo harness around the ESN detector: the callers either side of the hot path
(SURVEY 8f), rebuilt batched and device-resident.

    LinkParams      constants of a driver configuration                                          link.py
                    (Demo_MIMO_4x8_Sionna_CDL_ESN_v2.py:182-238, :285-288)
    FrameSource     (frames.py, with the channel record: percentiles_linear, summarize_channel_metrics)
                    bits -> QAM -> N*ifft -> CP -> sqrt(Pi) -> PA -> per-link 8-tap FIR -> AWGN
                    (:323-356 pilot, :397-427 data), TDL-B taps (:127-177) or the exponential-PDP
                    Rayleigh taps of OFDM_MIMO_2-2_NBF_LDPC.py:162-164,272-279: HIP kernels
                    (esn_gen_taps / esn_gen_frames, csrc/esn_gen.hip) with Philox counter streams keyed
                    by (seed, snr index, global block / frame index), so a block is identical on any rank.
    DetectorSweep   (sweep.py, with draw_reservoir, blocks_for_rank, reduce_counters)
                    per SNR point: G coherence blocks at a time -> one harvest + one solve launch
                    (training, helper_mimo_esn_generic.py:58-86), one predict launch over G*L data
                    frames, one fused detect/count launch; int64 counters [n_snr, {err, bits}]
                    reduced over ranks with a single all_reduce (RCCL) at the end.
    coded_ber_point, block_fading_point
                    one Eb/No point of the coded comparisons of the drivers                      points.py
    baseline_tracking_point
                    the LS-MMSE baseline of one Eb/No point with its channel estimate re-made after    points.py
                    every data symbol (FrameSource.track_channel, esn_channel_track)
    elm_point       one Eb/No point of the windowed ELM (elm.py, esn_elm_features / esn_elm_predict), the          points.py
                    reference's pinv-trained comparator, on the frames a DetectorSweep of the same seed detects
    fnn_point       the same for the windowed FNN (fnn.py, esn_fnn_train / esn_fnn_predict), the reference's          points.py
                    Adam-trained comparator: one training per block, all 50 epochs in one launch; the chunk loop is
                    elm_point's (points._windowed_point over points._chunks and frames.pilot_rows); what the three
                    Adam-trained points share -- optimiser and shape checks, shared or per-block initial sets, the
                    training of a chunk -- is points._trained_point over a trained.TrainedBank
    cnn_point       the same for the windowed CNN (cnn.py, esn_cnn_train / esn_cnn_predict), the reference's          points.py
                    three-layer Conv1d comparator, float64 throughout
    lstm_point      the same for the LSTM (lstm.py, esn_lstm_train / esn_lstm_predict), the reference's recurrent          points.py
                    comparator (its RNN curve), float64 throughout
    ensemble_point  one Eb/No point of a reservoir ensemble (ensemble.py, esn_detect_count_ens): K small ESNs per          points.py
                    block, each fitted on the block's pilot, outputs averaged before the FFT; member 0 is the ESN of a
                    DetectorSweep of the same seed (sweep.reservoir_seed, host_reservoir_bank, fit_e_dtype); a flagged fit
                    has it, elm_point or equalized_esn_point redone with the QR solve (points._retry_with_qr)
    equalized_esn_point  one Eb/No point of a small ESN behind the LS-MMSE equaliser (FrameSource.equalize_rows,          points.py
                    esn_mmse_equalize_rows): the equalised signal back in the time domain is the reservoir's input
    coded_equalized_point  its coded leg: coded_ber_point's payloads through that chain and the fused soft tail          points.py
                    (detect_llr, esn_detect_llr), LLRs flat or weighted by the equaliser's SINR (FrameSource.mmse_sinr)
    dcc_point       one Eb/No point of the amplifier-aware LS-MMSE baseline (FrameSource.mmse_dcc_detect_count,          points.py
                    esn_mmse_dcc_detect_count): decision-aided cancellation of the amplifier's distortion, on the frames
                    and the channel estimate of equalized_esn_point

The reference redraws a reservoir per coherence block from the global RNG; the sweep
supports that ("per_block" reservoirs from a pre-drawn pool) and the shared-reservoir mode the
throughput target assumes.

This module is the import path of all of them; the code lives in the four modules named above.
"""
from .frames import FrameSource, _view_real, complex_as_io, percentiles_linear, summarize_channel_metrics  # noqa: F401
from .link import LinkParams  # noqa: F401
from .points import baseline_tracking_point, block_fading_point, coded_ber_point, elm_point  # noqa: F401
from .points import fnn_point, fnn_weights  # noqa: F401
from .points import cnn_point, cnn_weights  # noqa: F401
from .points import lstm_point, lstm_weights  # noqa: F401
from .points import ensemble_point  # noqa: F401
from .points import equalized_esn_point  # noqa: F401
from .points import coded_equalized_point  # noqa: F401
from .points import dcc_point  # noqa: F401
from .sweep import DetectorSweep, blocks_for_rank, draw_reservoir, reduce_counters, stream_seed  # noqa: F401
