// gauss_window.h - the SSIM window that train.hip (the training loss) and metrics.hip (the evaluation metrics) filter with.
#pragma once

// pytorch_msssim._fspecial_gauss_1d(11, 1.5) as torch evaluates it in float32 (exp(-(i-5)^2 / 4.5), normalised by the
// float32 sum): the eleven values the reference's SSIM module holds, as literals
#define TS_GAUSS_WINDOW 0x1.0d957p-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f, \
                        0x1.b43c3ep-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d957p-10f
