"""What the interactive front-ends share - drop-in for reversi_zero/play_game/common.py."""
from ..lib.model_helpler import load_best_model_weight, reload_newest_next_generation_model_if_changed


def load_model(config):
    """common.py:5-14: the newest next_generation model where config.play.use_newest_next_generation_model says so and one
    exists, else the best model (and the other way round); RuntimeError when neither is there."""
    from ..agent.model import ReversiModel
    model = ReversiModel(config)
    order = (reload_newest_next_generation_model_if_changed, load_best_model_weight)
    if not config.play.use_newest_next_generation_model:
        order = order[::-1]
    if not (order[0](model) or order[1](model)):
        raise RuntimeError("No models found!")
    return model
