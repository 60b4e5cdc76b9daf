"""Host restatement of the two state rewards the device rollout evaluates (csrc/pyz_pilco.h, PYZ_REWARD_*), written from
their formulas; ``all_rewards`` maps the reference's names to them.  Each takes states with the state entries on the last
axis and the time step t, and works on one state or on a batch."""

import numpy as np

CART_ANGLE_LIMIT = 0.2095      # radians: the pole angle at which a CartPole episode ends


def cart_reward(s, t):
    """r = -s2 - s3 s2 + t (-s2^2 + 0.2095^2): s2 the pole's angle, s3 its angular velocity."""
    s = np.asarray(s)
    angle, spin = s[..., 2], s[..., 3]
    return -angle * (1.0 + spin) + t * (CART_ANGLE_LIMIT ** 2 - angle ** 2)


def acrobot_reward(s, t):
    """r = 4 - 3 s0 - (s0 s2 - s1 s3) + s4^2: (s0, s1) and (s2, s3) the cosines and sines of the two joint angles, s4 the
    first joint's angular velocity."""
    s = np.asarray(s)
    c1, s1, c2, s2, w1 = (s[..., k] for k in range(5))
    return 4.0 - 3.0 * c1 - (c1 * c2 - s1 * s2) + w1 ** 2


all_rewards = {"Acb 2 factors": acrobot_reward, "Cart": cart_reward}
MIN_STATE = {"Acb 2 factors": 5, "Cart": 4}     # state entries each one reads
