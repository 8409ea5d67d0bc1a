"""What the two Tacotron streaming test files share: the postnet shapes with the halo each must have, and weights that never stop.
Nothing here touches a GPU."""
import numpy as np

from tacotronv2_wavernn_chinese_amd.synth import make_tacotron_state
from tests import tacotron_fixtures as fx

# name -> (dims, halo): layers x taps; an even kernel puts its extra tap on the right ('same' padding: (k - 1) // 2 on the left)
POSTNET_SHAPES = {
    '5x5': (fx.SMALL, 10),
    '2x3': (dict(fx.SMALL, postnet_layers=2, postnet_kernel=3), 2),
    '2x4': (dict(fx.SMALL, postnet_layers=2, postnet_kernel=4), 4),
    '1x5': (dict(fx.SMALL, postnet_layers=1, postnet_kernel=5), 2),
    '5x5_r2': (fx.SMALL2, 10),
}
SEED = 3


def never_stopping_state(dims, seed=SEED):
    """Seeded weights with the stop projection's bias lowered by 64, as craft_stop does for its probe run: no stop token exceeds 0.5."""
    state = dict(make_tacotron_state(seed, **dims))
    state[fx.STOP] = (state[fx.STOP] - np.float32(64.0)).astype(np.float32)
    return state
