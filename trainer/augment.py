from cta_gan_amd.trainer.augment import *  # noqa: F401,F403
