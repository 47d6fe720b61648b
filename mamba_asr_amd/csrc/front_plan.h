// front_plan.h — what the two streamed front-end files (fbank_fft.hip, cnn_front.hip) agree on.
#pragma once

// Columns of the (batch, PL_W) int32 plan table of the per-slot entry points (cm_fbank_wav_stream_slots, cm_fbank_finish_stream_slots,
// cm_cnn_front_stream_slots): row b holds what the lock-step struct holds once for all streams.  The entry point checks a host copy,
// the kernel reads a device copy.
enum { PL_N = 0, PL_CONSUMED = 1, PL_TOTAL = 2, PL_F0 = 3, PL_NF = 4, PL_R0 = 5, PL_NR = 6, PL_TTOTAL = 7, PL_W = 8 };

// Feature rows of history per stream: cm_fbank_finish_stream writes them, cm_cnn_front_stream reads them (a row reaches back at most 6).
constexpr int FH = 8;
