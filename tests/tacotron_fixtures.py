"""The fixtures the Tacotron tests share: seeded weights, symbol sequences and targets, the float64 and float32 restatements of each,
the unit g of every quantity and the lead of every discrete decision.  test_tacotron_host.py qualifies each fixture on the CPU;
test_gpu_tacotron.py runs the kernels on exactly these.  Nothing here touches a GPU."""
import functools

import numpy as np

from tests import tacotron_ref as ref
from tacotronv2_wavernn_chinese_amd.synth import make_tacotron_state
from tacotronv2_wavernn_chinese_amd.tacotron import DEFAULT_TACOTRON_DIMS

REF = dict(n_symbols=40)                       # the reference's hparams (the symbol table's size is the data's, not the model's)
SMALL = dict(n_symbols=30, num_mels=20, embedding_dim=24, enc_conv_channels=40, enc_conv_kernel=5, encoder_lstm_units=20, attention_dim=24,
             attention_filters=6, attention_kernel=7, prenet_layers=(24, 16), decoder_lstm_units=36, postnet_channels=40)
SMALL2 = dict(SMALL, outputs_per_step=2)
MARGIN = 1000.0                                # every decision leads by at least MARGIN g (the precedent of test_align_host.py)
STOP = 'decoder/stop_token_projection/projection_stop_token_projection/bias'

# name -> dims, Tx, steps (decoder steps: the target's with 'gta', max_iters when free-running), mode, stop ('never', or 'mid': the stop
# projection's bias is set so that the float64 run stops at a step s with 5 <= s <= steps - 5), the seeds (picked on the CPU so that the
# fixture qualifies; test_tacotron_host.py asserts that it does), variant of the weights, prenet dropout
FIXTURES = {
    'ref_gta':      dict(dims=REF, Tx=63, steps=24, mode='gta', stop=None, seed=1, variant='default', dropout=True),
    'ref_stop':     dict(dims=REF, Tx=31, steps=24, mode='free', stop='mid', seed=302, variant='peaked', dropout=True),
    'ref_max':      dict(dims=REF, Tx=200, steps=2, mode='free', stop='never', seed=3, variant='default', dropout=True),
    'small_gta':    dict(dims=SMALL, Tx=65, steps=24, mode='gta', stop=None, seed=4, variant='peaked', dropout=True),
    'small2_gta':   dict(dims=SMALL2, Tx=64, steps=24, mode='gta', stop=None, seed=5, variant='default', dropout=True),
    'small_tx1':    dict(dims=SMALL, Tx=1, steps=1, mode='free', stop='never', seed=6, variant='default', dropout=True),
    'small2_tx2':   dict(dims=SMALL2, Tx=2, steps=2, mode='free', stop='never', seed=7, variant='default', dropout=True),
    'small_tx5':    dict(dims=SMALL, Tx=5, steps=24, mode='free', stop='never', seed=8, variant='default', dropout=True),
    'small2_stop':  dict(dims=SMALL2, Tx=31, steps=24, mode='free', stop='mid', seed=9, variant='default', dropout=True),
    'small_nodrop': dict(dims=SMALL, Tx=31, steps=24, mode='gta', stop=None, seed=10, variant='default', dropout=False),
}
FLOATS = ('encoder_outputs', 'decoder_output', 'alignments', 'stop', 'mel_raw', 'mel')   # compared as error <= K g
INTS = ('max_attentions', 'steps', 'mel_length')                                            # compared exactly


def full_dims(dims):
    d = dict(DEFAULT_TACOTRON_DIMS)
    d.update(dims)
    return d


def ref_kwargs(dims):
    d = full_dims(dims)
    return dict(num_mels=d['num_mels'], r=d['outputs_per_step'], prenet_sizes=tuple(d['prenet_layers']), decoder_layers=d['decoder_layers'],
                enc_conv_layers=d['enc_conv_layers'], postnet_layers=d['postnet_layers'], zoneout=d['zoneout'])


def run_ref(state, dims, seq, dtype, **kw):
    return ref.synthesize(state, seq, dtype, **ref_kwargs(dims), **kw)


def craft_stop(state, dims, seq, seed, steps, how, dropout=True):
    """Shift the stop projection's bias by one number: 'never' puts every logit of the float64 run at -2 or below; 'mid' puts the bias
    half-way between the logit of the first step s in 5 .. steps - 5 that exceeds every earlier one and the largest earlier one, so the run
    stops at s.  The decoder's trajectory does not depend on the stop token, so one float64 run gives all the logits.  Returns s or None."""
    never = dict(state)
    never[STOP] = state[STOP] - np.float32(64.0)
    z = run_ref(never, dims, seq, np.float64, max_iters=steps, seed=seed, prenet_dropout=dropout)['stop_logit'].max(axis=1) + 64.0
    if how == 'never':
        state[STOP] = (state[STOP] - np.float32(z.max() + 2.0)).astype(np.float32)
        return None
    for s in range(5, steps - 4):
        if z[s] > z[:s].max():
            state[STOP] = (state[STOP] - np.float32(0.5 * (z[s] + z[:s].max()))).astype(np.float32)
            return s
    raise AssertionError('no step in 5 .. steps - 5 whose stop logit exceeds every earlier one: pick another seed')


def decision_leads(r64, free):
    """The lead of every discrete decision of the float64 run, each as (kind, step, lead, quantity it rests on)."""
    out = []
    prev = 0
    for s in range(r64['steps']):
        f = r64['forward'][s]
        if prev + 1 < len(f):
            out.append(('argmax', s, abs(f[:prev + 1].max() - f[prev + 1:].max()), 'forward'))
        prev = int(r64['max_attentions'][s])
    if free:
        for i, p in enumerate(r64['stop']):
            out.append(('stop', i, abs(p - 0.5), 'stop'))
    return out


@functools.lru_cache(maxsize=None)
def fixture(name):
    """dict: state, seq, target, seed, kw (the restatement's arguments), r64, r32, g (quantity -> max |float32 - float64|), leads."""
    f = FIXTURES[name]
    dims, d = f['dims'], full_dims(f['dims'])
    rng = np.random.Generator(np.random.PCG64(1000 + f['seed']))
    state = dict(make_tacotron_state(f['seed'], f['variant'], **dims))
    seq = rng.integers(0, d['n_symbols'], size=f['Tx']).tolist()
    seed = 77 + f['seed']
    target, stop_step = None, None
    if f['mode'] == 'gta':
        target = rng.uniform(-4.0, 4.0, size=(f['steps'] * d['outputs_per_step'], d['num_mels'])).astype(np.float32)
        kw = dict(gta_target=target, seed=seed, prenet_dropout=f['dropout'])
    else:
        stop_step = craft_stop(state, dims, seq, seed, f['steps'], f['stop'], f['dropout'])
        kw = dict(max_iters=f['steps'], seed=seed, prenet_dropout=f['dropout'])
    r64, r32 = run_ref(state, dims, seq, np.float64, **kw), run_ref(state, dims, seq, np.float32, **kw)
    g = {}
    for q in FLOATS + ('forward',):
        g[q] = float(np.max(np.abs(r32[q].astype(np.float64) - r64[q]))) if r32[q].shape == r64[q].shape else float('inf')
    return dict(f, name=name, state=state, seq=seq, target=target, seed=seed, kw=kw, r64=r64, r32=r32, g=g, stop_step=stop_step,
                leads=decision_leads(r64, f['mode'] == 'free'), full=d)
