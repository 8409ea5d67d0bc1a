// Host only (dsp_tables.h): the window, twiddle, filterbank and DCT tables every analysis family reads.  No kernels here.
#include "dsp_tables.h"

#include <cmath>

namespace wrnn_dsp {

namespace {
const double PI = 3.141592653589793;
const double F_SP = 200.0 / 3.0, MIN_LOG_HZ = 1000.0;
}  // namespace

std::vector<double> hann_periodic(int win) {
    std::vector<double> w(win);
    const double wstep = (PI - (-PI)) / (double)win;
    for (int i = 0; i < win; ++i) w[i] = 0.5 + 0.5 * std::cos((double)i * wstep + (-PI));
    return w;
}

std::vector<double> twiddles(int n_fft) {
    std::vector<double> t(2 * (size_t)n_fft);
    for (int k = 0; k < n_fft; ++k) {
        const double ang = 2.0 * PI * (double)k / (double)n_fft;
        t[2 * k] = std::cos(ang);
        t[2 * k + 1] = -std::sin(ang);
    }
    return t;
}

std::vector<double> np_linspace(double start, double stop, int num) {
    std::vector<double> y(num);
    const double step = (stop - start) / (double)(num - 1);
    for (int i = 0; i < num; ++i) y[i] = (double)i * step + start;
    y[num - 1] = stop;
    return y;
}

double hz_to_mel(double f) {
    const double min_log_mel = MIN_LOG_HZ / F_SP, logstep = std::log(6.4) / 27.0;
    return f >= MIN_LOG_HZ ? min_log_mel + std::log(f / MIN_LOG_HZ) / logstep : f / F_SP;
}

double mel_to_hz(double m) {
    const double min_log_mel = MIN_LOG_HZ / F_SP, logstep = std::log(6.4) / 27.0;
    return m >= min_log_mel ? MIN_LOG_HZ * std::exp(logstep * (m - min_log_mel)) : F_SP * m;
}

std::vector<double> slaney_basis(int sample_rate, int n_fft, int n_mels, double fmin, double fmax_arg) {
    const int NB = n_fft / 2 + 1;
    const double nyquist = 0.5 * (double)sample_rate, fmax = fmax_arg == 0.0 ? nyquist : fmax_arg;
    const std::vector<double> fftfreqs = np_linspace(0.0, nyquist, NB);
    std::vector<double> mel_f = np_linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2);
    for (double &m : mel_f) m = mel_to_hz(m);
    std::vector<double> basis((size_t)n_mels * NB);
    for (int i = 0; i < n_mels; ++i) {
        const double fd0 = mel_f[i + 1] - mel_f[i], fd1 = mel_f[i + 2] - mel_f[i + 1], enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
        for (int k = 0; k < NB; ++k) {
            const double lower = -(mel_f[i] - fftfreqs[k]) / fd0, upper = (mel_f[i + 2] - fftfreqs[k]) / fd1;
            basis[(size_t)i * NB + k] = std::fmax(0.0, std::fmin(lower, upper)) * enorm;
        }
    }
    return basis;
}

std::vector<double> dct_rows(int n_mels, int K) {
    const double scale = std::sqrt(2.0 / (double)n_mels);
    std::vector<double> dct((size_t)K * n_mels);
    for (int k = 1; k <= K; ++k)
        for (int m = 0; m < n_mels; ++m) dct[(size_t)(k - 1) * n_mels + m] = scale * std::cos(PI * (double)k * ((double)m + 0.5) / (double)n_mels);
    return dct;
}

}  // namespace wrnn_dsp
