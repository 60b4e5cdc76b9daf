"""What SGD and SWAG share for n_members = P > 1 (an extension: the reference trains one model per optimizer): the
members' starting points (with P = 1: the one model's, as the reference copies it)."""

import numpy as np


def n_members_of(kwargs) -> int:
    P = int(kwargs.get("n_members", 1))
    if P < 1:
        raise ValueError("n_members must be at least 1")
    return P


def check_starts(start, P: int):
    """A list or tuple of starting models has one entry per member (checked before any device work)."""
    if isinstance(start, (list, tuple)) and len(start) != P:
        raise ValueError(f"starting_model lists {len(start)} models for n_members = {P}")


def member_starts(opt, start, P: int) -> np.ndarray:
    """(P, D) float32.  A list or tuple of P models: member c copies entry c (the MultiSWAG recipe:
    SWAG(starting_model=sgd.member_models())).  One model: member 0 copies it, as the one-member optimizer does, and
    member c >= 1 takes reset_glorot(default_rng(seed + c)), the rule of SGLD's chains -- the reference's starting_model
    is in practice a freshly built, randomly initialised Keras model.  opt._net is left with member 0's weights."""
    from ..nn.model import model_from_json
    rows = []
    for c in range(P):
        scratch = model_from_json(opt._model_config)
        if isinstance(start, (list, tuple)):
            scratch.set_weights(start[c].get_weights())
        elif c == 0:
            scratch.set_weights(start.get_weights())
        else:
            scratch.reset_glorot(np.random.default_rng(opt._seed + c))
        rows.append(scratch.weights_flat.copy())
    opt._net.set_flat(rows[0])
    return np.stack(rows).astype(np.float32)

