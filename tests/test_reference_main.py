"""nfsp_amd.reference_main, the launcher for the reference's own main.py (CPU part).

`reference_main.run` supplies the host-side modules main.py imports besides the drop-in
(tensorflow, matplotlib.pyplot, ConfigParser) and runs the file as __main__ in its own
directory.  The reference's main.py is not part of this repository, so nothing here runs it:
these tests cover the stand-ins and the command line; the GPU suite runs the launcher end to
end on a driver written for it (tests/test_gpu_dropin.py).
"""


def test_stubs_cover_what_main_py_uses(pkg):
    rm = pkg.reference_main
    tf = rm.tensorflow_stub()
    with tf.Session() as sess:
        assert sess.run(tf.global_variables_initializer()) is None
    assert sess.closed
    tf.set_random_seed(1234)
    assert tf.seeds == [1234]
    mpl, plt = rm.matplotlib_stub()
    plt.plot([1.0, 2.0])
    plt.show()
    assert plt.curves == [[1.0, 2.0]] and plt.shown == 1 and mpl.pyplot is plt
    import time
    ts = rm.time_stub()
    assert ts.sleep(60) is None and ts.time is time.time and time.sleep is not ts.sleep
    # only code run with main_builtins gets the stub; sys.modules keeps the real module
    import sys
    g = {"__builtins__": rm.main_builtins(ts)}
    exec("import time\nimport os\ndef f():\n    import time as t\n    return t", g)
    assert g["time"] is ts and g["f"]() is ts and g["os"] is sys.modules["os"]
    assert sys.modules["time"] is time
    cp = rm.configparser_stub({("Common", "Episodes"): 7}).ConfigParser()
    cp.read_string("[Common]\nEpisodes: 400000\n[Agent]\nEta: 0.1\n")
    assert cp.get("Common", "Episodes") == "7" and cp.get("Agent", "Eta") == "0.1"


def test_cli_splits_its_own_options_from_main_py_args(pkg, monkeypatch):
    seen = {}

    def fake_run(main_py, episodes=None, argv=(), skip_sleep=True, plot_to=None, **kw):
        seen.update(main_py=main_py, episodes=episodes, argv=list(argv), skip_sleep=skip_sleep, plot_to=plot_to)
        return {"curves": [], "tf_seeds": [], "globals": {}}

    monkeypatch.setattr(pkg.reference_main, "run", fake_run)
    assert pkg.reference_main.main(["m.py", "--episodes", "10", "--plot-to", "c", "--", "--human"]) == 0
    assert seen == dict(main_py="m.py", episodes=10, argv=["--human"], skip_sleep=True, plot_to="c")
    pkg.reference_main.main(["m.py", "--sleep"])
    assert seen["argv"] == [] and seen["episodes"] is None and not seen["skip_sleep"]
