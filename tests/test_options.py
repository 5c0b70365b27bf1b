"""The options record (src/dalle_mtf/options.py) on the CPU: every field against its module's resolver, the order of the errors,
the checkpoint entries and the checkpoint check against the literal messages, the logged lines and generate.json's fields."""
import itertools

import pytest

from src.dalle_mtf import options as O
from src.dalle_mtf.activations import resolve_activation
from src.dalle_mtf.dropout import resolve_dropout
from src.dalle_mtf.ema import resolve_ema
from src.dalle_mtf.ff_glu import resolve_ff_glu
from src.dalle_mtf.loss_weights import resolve_loss_weights
from src.dalle_mtf.qk_norm import resolve_qk_norm
from src.dalle_mtf.rotary import resolve_rotary
from src.dalle_mtf.token_shift import resolve_token_shift

D, H, T, P = 512, 4, 256, 1024            # configs/dalle_example.json: a 32 x 32 image grid, heads of 128
ABSENT = "absent"
MODEL_FIELDS = ("activation", "rotary", "rotary_base", "token_shift", "ff_glu", "qk_norm")


def _opt(**params):
    return O.resolve_options(params, D, T, P)


def _params(**kv):
    return {k: v for k, v in kv.items() if v is not ABSENT}


GRID = [_params(activation_fn=act, rotary_emb=rot, rotary_base=base, token_shift=ts, ff_glu=glu, qk_norm=qk)
        for act, (rot, base), ts, glu, qk in itertools.product(
            (ABSENT, None, "relu", "gelu"),
            ((ABSENT, ABSENT), (None, ABSENT), (False, 500.0), ("1d", ABSENT), ("1d", 500.0), ("axial", ABSENT), ("axial", 123)),
            (ABSENT, None, False, True), (ABSENT, None, False, True), (ABSENT, None, False, True))]
TRAINING = [{}, dict(text_loss_weight=1, image_loss_weight=7), dict(image_loss_weight=0.5), dict(ema_decay=0.99),
            dict(ema_decay=0.999, ema_eval=True), dict(ema_decay=0, ema_eval=False), dict(embed_dropout=0.1),
            dict(residual_dropout=0.25, dropout_seed=7), dict(embed_dropout=0.1, residual_dropout=0.1, dropout_seed=3,
                                                              text_loss_weight=2.0, ema_decay=0.9)]


def _by_module(params, activation_fn=None):
    rot = resolve_rotary(params, P)
    return O.Options(resolve_activation(activation_fn, params), rot[0], rot[1], resolve_token_shift(params, D, P), resolve_ff_glu(params),
                     resolve_qk_norm(params), resolve_loss_weights(params, T), *resolve_ema(params), *resolve_dropout(params))


def test_every_field_is_its_modules_resolver():
    assert len(GRID) == 4 * 7 * 64
    assert O.Options._fields == MODEL_FIELDS + ("loss_weights", "ema_decay", "ema_eval", "embed_thresh", "resid_thresh", "dropout_seed")
    for params in GRID:
        assert O.resolve_options(params, D, T, P) == _by_module(params), params
    for extra in TRAINING:
        for params in GRID[::97]:
            params = dict(params, **extra)
            assert O.resolve_options(params, D, T, P) == _by_module(params), params
    assert O.resolve_options(None, D, T, P) == _by_module(None) == _opt()
    # the argument goes before the config key
    assert O.resolve_options({"activation_fn": "relu"}, D, T, P, activation_fn="gelu").activation == "gelu"
    assert O.resolve_options({"activation_fn": "gelu"}, D, T, P, activation_fn=None).activation == "gelu"


def test_defaults_and_one_full_record():
    assert _opt() == O.Options("relu", None, 10000.0, False, False, False, None, None, False, 0, 0, 0)
    on = _opt(activation_fn="gelu", rotary_emb="axial", rotary_base=500, token_shift=True, ff_glu=True, qk_norm=True,
              text_loss_weight=1, image_loss_weight=7, ema_decay=0.99, ema_eval=True, embed_dropout=0.5, residual_dropout=0.25, dropout_seed=9)
    assert on == O.Options("gelu", "axial", 500.0, True, True, True, (1.0, 7.0), 0.99, True, 32768, 16384, 9)
    with pytest.raises(AttributeError):
        on.ff_glu = False


# the resolvers in DALLE's order, each with a bad value of its key and a word of its error
BAD = [("activation_fn", "silu", NotImplementedError, "activation_fn"), ("text_loss_weight", -1, ValueError, "text_loss_weight"),
       ("ema_decay", 1.5, ValueError, "ema_decay"), ("embed_dropout", 1.0, ValueError, "embed_dropout"),
       ("rotary_emb", "2d", ValueError, "rotary_emb"), ("token_shift", 1, ValueError, "token_shift"),
       ("ff_glu", "yes", ValueError, "ff_glu"), ("qk_norm", 1, ValueError, "qk_norm")]


@pytest.mark.parametrize("first,second", list(itertools.combinations(range(len(BAD)), 2)))
def test_two_bad_keys_raise_the_earlier_ones_error(first, second):
    (k1, v1, exc, word), (k2, v2, _, _) = BAD[first], BAD[second]
    for params in ({k1: v1, k2: v2}, {k2: v2, k1: v1}):
        with pytest.raises(exc, match=word):
            O.resolve_options(params, D, T, P)


def test_the_shape_checks_are_the_modules():
    with pytest.raises(ValueError, match="rotary_emb: 'axial' needs image_seq_len to be a perfect square"):
        O.resolve_options({"rotary_emb": "axial"}, D, T, 1000)
    with pytest.raises(ValueError, match="token_shift: needs image_seq_len to be a perfect square"):
        O.resolve_options({"token_shift": True}, D, T, 1000)
    with pytest.raises(ValueError, match="token_shift: needs n_embd to be a multiple of 32"):
        O.resolve_options({"token_shift": True}, 48, T, P)
    with pytest.raises(ValueError, match="text_seq_len must be >= 2"):
        O.resolve_options({"text_loss_weight": 1}, D, 1, P)


# ------------------------------------------------------------------ checkpoints
def test_checkpoint_entries():
    assert O.checkpoint_entries(_opt()) == {"activation_fn": "relu"}
    assert O.checkpoint_entries(_opt(activation_fn="gelu")) == {"activation_fn": "gelu"}
    assert O.checkpoint_entries(_opt(rotary_emb="1d")) == {"activation_fn": "relu", "rotary_emb": "1d", "rotary_base": 10000.0}
    assert O.checkpoint_entries(_opt(rotary_emb="axial", rotary_base=500)) == {"activation_fn": "relu", "rotary_emb": "axial", "rotary_base": 500.0}
    assert O.checkpoint_entries(_opt(rotary_base=500)) == {"activation_fn": "relu"}          # a base without a scheme: nothing to record
    assert O.checkpoint_entries(_opt(token_shift=True)) == {"activation_fn": "relu", "token_shift": True}
    assert O.checkpoint_entries(_opt(ff_glu=True)) == {"activation_fn": "relu", "ff_glu": True}
    assert O.checkpoint_entries(_opt(qk_norm=True)) == {"activation_fn": "relu", "qk_norm": True}
    everything = O.checkpoint_entries(_opt(activation_fn="gelu", rotary_emb="axial", token_shift=True, ff_glu=True, qk_norm=True,
                                           ema_decay=0.9, embed_dropout=0.1, text_loss_weight=2))      # training options leave no entry
    assert everything == {"activation_fn": "gelu", "rotary_emb": "axial", "rotary_base": 10000.0, "token_shift": True, "ff_glu": True,
                          "qk_norm": True}
    assert list(everything) == ["activation_fn", "rotary_emb", "rotary_base", "token_shift", "ff_glu", "qk_norm"]
    for v in ("token_shift", "ff_glu", "qk_norm"):
        assert everything[v] is True


TAIL = ": the weights of one do not compute the other"
# (the checkpoint's model, the run's model, the message)
MISMATCHES = [
    (dict(activation_fn="gelu"), {}, "checkpoint was written by a gelu model; this run uses activation_fn 'relu'" + TAIL),
    ({}, dict(activation_fn="gelu"), "checkpoint was written by a relu model; this run uses activation_fn 'gelu'" + TAIL),
    ({}, dict(rotary_emb="axial"), "checkpoint was written by a model with no rotary embeddings; this run uses rotary_emb 'axial' "
                                   "(rotary_base 10000)" + TAIL),
    (dict(rotary_emb="axial"), {}, "checkpoint was written by a model with rotary_emb 'axial' (rotary_base 10000); this run uses "
                                   "no rotary embeddings" + TAIL),
    (dict(rotary_emb="axial"), dict(rotary_emb="1d"), "checkpoint was written by a model with rotary_emb 'axial' (rotary_base 10000); "
                                                      "this run uses rotary_emb '1d' (rotary_base 10000)" + TAIL),
    (dict(rotary_emb="axial"), dict(rotary_emb="axial", rotary_base=500.0),
     "checkpoint was written by a model with rotary_emb 'axial' (rotary_base 10000); this run uses rotary_emb 'axial' (rotary_base 500)" + TAIL),
    (dict(token_shift=True), {}, "checkpoint was written by a model with token_shift on; this run uses no token shift" + TAIL),
    ({}, dict(token_shift=True), "checkpoint was written by a model with no token shift; this run uses token_shift on" + TAIL),
    (dict(ff_glu=True), {}, "checkpoint was written by a model with ff_glu on (the gated FFN); this run uses ff_glu off (the plain FFN)" + TAIL),
    ({}, dict(ff_glu=True), "checkpoint was written by a model with ff_glu off (the plain FFN); this run uses ff_glu on (the gated FFN)" + TAIL),
    (dict(qk_norm=True), {}, "checkpoint was written by a model with qk_norm on (normalised q and k with learned gains); this run uses "
                             "qk_norm off (plain q and k)" + TAIL),
    ({}, dict(qk_norm=True), "checkpoint was written by a model with qk_norm off (plain q and k); this run uses qk_norm on (normalised q and "
                             "k with learned gains)" + TAIL),
]


@pytest.mark.parametrize("theirs,mine,message", MISMATCHES)
def test_check_checkpoint_messages_are_the_literal_ones(theirs, mine, message):
    sd = dict(O.checkpoint_entries(_opt(**theirs)), p=None, global_step=3, optimizer="adam")
    with pytest.raises(ValueError) as e:
        O.check_checkpoint(_opt(**mine), sd)
    assert str(e.value) == message
    O.check_checkpoint(_opt(**theirs), sd)                 # ... and its own model takes it
    O.check_checkpoint(_opt(ema_decay=0.9, residual_dropout=0.1, image_loss_weight=3, **theirs), sd)      # whatever the training options


def test_a_checkpoint_without_the_keys_is_an_all_off_relu_model():
    old = {"p": None, "global_step": 0}
    O.check_checkpoint(_opt(), old)
    O.check_checkpoint(_opt(activation_fn="relu", rotary_emb=False, token_shift=None, ff_glu=False), old)
    for on, word in ((dict(activation_fn="gelu"), "a relu model"), (dict(rotary_emb="1d"), "no rotary embeddings; this run uses rotary_emb '1d'"),
                     (dict(token_shift=True), "no token shift;"), (dict(ff_glu=True), "ff_glu off (the plain FFN);"),
                     (dict(qk_norm=True), "qk_norm off (plain q and k);")):
        with pytest.raises(ValueError, match="checkpoint was written by") as e:
            O.check_checkpoint(_opt(**on), old)
        assert word in str(e.value), str(e.value)
    # a recorded base without a scheme is not read; a base recorded as an int compares as a float
    O.check_checkpoint(_opt(), dict(old, rotary_base=500))
    O.check_checkpoint(_opt(rotary_emb="1d", rotary_base=500.0), dict(old, rotary_emb="1d", rotary_base=500))
    with pytest.raises(ValueError, match="rotary_base 10000\\); this run uses rotary_emb '1d' \\(rotary_base 500\\)"):
        O.check_checkpoint(_opt(rotary_emb="1d", rotary_base=500.0), dict(old, rotary_emb="1d"))      # no base recorded: the default


ORDER = [(dict(activation_fn="gelu"), "gelu model"), (dict(rotary_emb="1d"), "rotary_emb '1d'"), (dict(token_shift=True), "token_shift on"),
         (dict(ff_glu=True), "ff_glu on"), (dict(qk_norm=True), "qk_norm on")]


@pytest.mark.parametrize("first,second", list(itertools.combinations(range(len(ORDER)), 2)))
def test_two_mismatches_raise_the_earlier_checks_message(first, second):
    (a, word), (b, other) = ORDER[first], ORDER[second]
    sd = O.checkpoint_entries(_opt(**a, **b))
    with pytest.raises(ValueError) as e:
        O.check_checkpoint(_opt(), sd)
    assert word in str(e.value) and other not in str(e.value), str(e.value)


# ------------------------------------------------------------------ what is logged and reported
def test_option_log_lines():
    assert O.option_log_lines(_opt(), D, H, T, P) == []
    assert O.option_log_lines(_opt(activation_fn="gelu", embed_dropout=0.1, rotary_base=500), D, H, T, P) == []
    every = _opt(text_loss_weight=1, image_loss_weight=7, ema_decay=0.99, rotary_emb="axial", token_shift=True, ff_glu=True, qk_norm=True)
    assert O.option_log_lines(every, D, H, T, P) == [
        "loss weights: text 1, image 7 -> loss = (1 * mean_text + 7 * mean_image) / 8 over 255 text and 1025 image positions",
        "weight EMA: ema_decay 0.99 (decay at step t = min(0.99, (1 + t) / (10 + t))), evaluation from the raw weights",
        "rotary embeddings: axial, base 10000 (in addition to the learned positions)",
        "token shift: on (behind norm_1 and norm_2 of every block, 32 x 32 image grid)",
        "gated feed-forward: on (ReGLU, mlp_linear_1 is [512, 4096])",
        "QK normalisation: on (RMS per head over 128 channels, eps 1e-6, gains [128] per layer)"]
    assert O.option_log_lines(_opt(ema_decay=0.999, ema_eval=True), D, H, T, P) == [
        "weight EMA: ema_decay 0.999 (decay at step t = min(0.999, (1 + t) / (10 + t))), evaluation from the averaged weights"]
    assert O.option_log_lines(_opt(image_loss_weight=0.5), D, H, T, P) == [
        "loss weights: text 1, image 0.5 -> loss = (1 * mean_text + 0.5 * mean_image) / 1.5 over 255 text and 1025 image positions"]
    assert O.option_log_lines(_opt(rotary_emb="1d", rotary_base=500), D, H, T, P) == [
        "rotary embeddings: 1d, base 500 (in addition to the learned positions)"]
    assert O.option_log_lines(_opt(activation_fn="gelu", ff_glu=True), D, H, T, P) == ["gated feed-forward: on (GEGLU, mlp_linear_1 is [512, 4096])"]
    assert O.option_log_lines(_opt(qk_norm=True), D, 8, T, P) == [
        "QK normalisation: on (RMS per head over 64 channels, eps 1e-6, gains [64] per layer)"]


def test_report():
    assert O.report(_opt()) == dict(rotary_emb=None, rotary_base=None, token_shift=False, ff_glu=False, qk_norm=False)
    assert O.report(_opt(rotary_base=500)) == dict(rotary_emb=None, rotary_base=None, token_shift=False, ff_glu=False, qk_norm=False)
    got = O.report(_opt(activation_fn="gelu", rotary_emb="axial", rotary_base=500, token_shift=True, ff_glu=True, qk_norm=True, ema_decay=0.9))
    assert got == dict(rotary_emb="axial", rotary_base=500.0, token_shift=True, ff_glu=True, qk_norm=True)
    assert list(got) == ["rotary_emb", "rotary_base", "token_shift", "ff_glu", "qk_norm"]
    assert O.report(_opt(rotary_emb="1d", qk_norm=True)) == dict(rotary_emb="1d", rotary_base=10000.0, token_shift=False, ff_glu=False, qk_norm=True)
