"""The four dim sets the WRNN_KERNEL_TEAMG tests run (tests/test_teamg_host.py, tests/test_gpu_teamg.py).

A   256 / 384 (test_gpu_any_dims.SMALL)      a small model: its loop weights are almost fully LDS resident
B   rnn 100, fc 72, feat 13, res_out 20       nothing divides by 32, 16 or 4; seven workgroups own no hidden unit, nine no fc row
C   1024 / 1024                               almost everything is streamed
D   DEFAULT_DIMS                              the reference hparams on the generic kernel
"""
from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS

DIM_SETS = {
    'A': dict(rnn_dims=256, fc_dims=384, bits=8, pad=2, upsample_factors=(4, 4, 8), feat_dims=40, compute_dims=64, res_out_dims=96,
              res_blocks=3, hop_length=128, sample_rate=16000),
    'B': dict(rnn_dims=100, fc_dims=72, bits=7, pad=2, upsample_factors=(2, 3), feat_dims=13, compute_dims=16, res_out_dims=20,
              res_blocks=1, hop_length=6, sample_rate=16000),
    'C': dict(rnn_dims=1024, fc_dims=1024, bits=10, pad=2, upsample_factors=(2, 3), feat_dims=80, compute_dims=128, res_out_dims=128,
              res_blocks=1, hop_length=6, sample_rate=22050),
    'D': dict(DEFAULT_DIMS),
}
LDS_BYTES = 160 * 1024


def layer_shapes(dims, mode='RAW'):
    """name -> (units, rows per unit, floats per row) of the six layers, from the constructor dims alone."""
    H, FC, F, A = dims['rnn_dims'], dims['fc_dims'], dims['feat_dims'], dims['res_out_dims'] // 4
    NC = 2 ** dims['bits'] if mode == 'RAW' else 30
    return {'fc3': (NC, 1, FC), 'fc2': (FC, 1, FC + A), 'fc1': (FC, 1, H + A), 'rnn2': (H, 3, 2 * H + A), 'rnn1': (H, 3, 2 * H), 'cond': (H, 1, F + A)}
