from cusrl_amd.hook.player.save_transition import SaveTransition

__all__ = ["SaveTransition"]
