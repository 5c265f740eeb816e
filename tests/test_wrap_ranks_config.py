"""EngineConfig.wrap_ranks / wrap_devices and the service's --wrap-ranks / --wrap-devices (no GPU): the Groth16 wrap over the ranks of a
communicator takes the same rank counts and device lists as the final STARK's final_ranks / final_devices."""
import sys

import pytest

from eigen_zeth_amd.service import __main__ as CLI
from eigen_zeth_amd.service.engine import EngineConfig


def test_engine_config_accepts_wrap_ranks_and_devices():
    assert EngineConfig().wrap_ranks == 1 and EngineConfig().wrap_devices is None
    for ranks in (1, 2, 4, 8, 64):
        cfg = EngineConfig(air="chunk64", logn=14, wrap_ranks=ranks)
        assert cfg.wrap_ranks == ranks and cfg.wrap_devices is None
    cfg = EngineConfig(air="chunk64", logn=14, wrap_ranks=4, wrap_devices=[0, 1, 2, 3])
    assert cfg.wrap_devices == [0, 1, 2, 3]


@pytest.mark.parametrize("ranks", [3, 0, 128, -2, True, 2.0, "2"])
def test_engine_config_refuses_bad_wrap_ranks(ranks):
    with pytest.raises(ValueError, match="wrap_ranks"):
        EngineConfig(air="chunk64", logn=14, wrap_ranks=ranks)


@pytest.mark.parametrize("devices", [[0], [0, 1, 2], [0, -1], [0, "1"]])
def test_engine_config_refuses_a_wrong_device_list(devices):
    with pytest.raises(ValueError, match="wrap_devices"):
        EngineConfig(air="chunk64", logn=14, wrap_ranks=2, wrap_devices=devices)


@pytest.mark.parametrize("argv", [["--wrap-ranks", "3"], ["--wrap-ranks", "0"], ["--wrap-ranks", "128"],
                                  ["--wrap-ranks", "2", "--wrap-devices", "0,1,2"], ["--wrap-ranks", "4", "--wrap-devices", "0"]])
def test_cli_refuses_the_same_values(monkeypatch, capsys, argv):
    monkeypatch.setattr(sys, "argv", ["eigen_zeth_amd.service"] + argv)
    monkeypatch.setattr(CLI, "serve", lambda *a, **k: pytest.fail("the service was started with %r" % (argv,)))
    with pytest.raises(SystemExit) as ei:
        CLI.main()
    assert ei.value.code == 2
    assert "--wrap-" in capsys.readouterr().err


def test_cli_hands_wrap_ranks_to_the_engine(monkeypatch):
    seen = {}

    class Stop(Exception):
        pass

    def serve(port, host, state_dir, cfg, device, **kw):
        seen["cfg"] = cfg
        raise Stop()
    monkeypatch.setattr(sys, "argv", ["eigen_zeth_amd.service", "--no-prewarm", "--wrap-ranks", "2", "--wrap-devices", "0,1"])
    monkeypatch.setattr(CLI, "serve", serve)
    with pytest.raises(Stop):
        CLI.main()
    assert seen["cfg"].wrap_ranks == 2 and seen["cfg"].wrap_devices == [0, 1]
