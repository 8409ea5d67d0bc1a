// The host tables of the analysis families (dsp_tables.hip), built in float64 and returned unrounded: a caller that wants float32
// (the mel front end, the score section's DCT) rounds once, itself.  Every expression follows NumPy's / librosa's evaluation order.
#pragma once
#include <vector>

namespace wrnn_dsp {

// scipy.signal.get_window('hann', win, fftbins=True): the symmetric window of win + 1 points without its last one
std::vector<double> hann_periodic(int win);
// [n_fft][2]: cos, -sin of 2 pi k / n_fft
std::vector<double> twiddles(int n_fft);
// np.linspace(start, stop, num), num >= 2: arange * step + start, last point set to stop
std::vector<double> np_linspace(double start, double stop, int num);
// Slaney mel scale (librosa htk=False): linear below 1 kHz, 200/3 Hz per mel; log above, 27 mels per factor 6.4
double hz_to_mel(double f);
double mel_to_hz(double m);
// librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax, htk=False, norm=1), dense (n_mels, n_fft / 2 + 1); fmax == 0: sample_rate / 2.
// The bin frequencies run to sample_rate / 2 whatever fmax is.
std::vector<double> slaney_basis(int sample_rate, int n_fft, int n_mels, double fmin, double fmax);
// (K, n_mels): C[k, m] = sqrt(2 / n_mels) cos(pi k (m + 1/2) / n_mels) for k = 1 .. K
std::vector<double> dct_rows(int n_mels, int K);

}  // namespace wrnn_dsp
